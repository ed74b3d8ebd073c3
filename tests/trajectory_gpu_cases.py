"""The cases of tests/test_gpu_trajectory.py, each run in a fresh process (`python tests/trajectory_gpu_cases.py <case>`): torch must
initialise its HIP runtime before the product library does (tests/test_gpu_boundary.py).  Not collected by pytest (no test_ prefix on
the file).  What is checked, and why each bound is what it is: DESIGN.md section 13."""
import itertools
import os
import sys

import torch

torch.cuda.init()      # first: the other order leaves torch without a device

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import end_velocity_ref as er  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from oracle_api import Oracle  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

DEV = "cuda:0"
NS = (1, 63, 64, 65, 255, 257, 4097)
KS = (1, 2, 33, 63, 64, 65, 200)
BIG = 4097
# beyond the grid's cap: at k = 1 and 2 a block takes 128 problems per trip, so 300,001 problems are 2,344 trips for the grid's 2,048 blocks,
# the last one partial and the total odd; the rows looked at are the first 257, those around problem 2,048 x 128 = 262,144, where the
# blocks start their second trip, and the last 257.  The kernels of the later sections -- k_gap, k_tracking with its vjp and jvp, k_meeting,
# k_separation, k_contact, k_fleet, k_encounter, k_stagger, k_rendezvous, k_reach (GRID_N pair problems; 100,001 scenes of three vehicles,
# 300,003 problems, the rows whole scenes) and k_shortlisted (a list longer than 262,144) -- have their cases on these rows in
# grid_cap_gpu_cases.py and shortlist_gpu_cases.py
GRID_N, GRID_KS = 300001, (1, 2)
GRID_ROWS = (slice(0, 257), slice(262016, 262401), slice(GRID_N - 257, GRID_N))
PAD, SENTINEL = 16, 7.0      # doubles behind every output buffer, and what they hold


def _t(a):
    """The array on the device, complete before it returns: a batch's stream is non-blocking, so nothing else orders torch's upload on the
    null stream before a kernel there."""
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)
    torch.cuda.synchronize()
    return t


def _bits(a):
    return np.atleast_1d(np.ascontiguousarray(a, dtype=np.float64)).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


class Out:
    """An output buffer of `shape` with PAD sentinel doubles behind it.  The fill is a kernel on torch's null stream and the batch entry
    writes on the batch's own non-blocking stream: the fill is waited for here, or it could land on top of the result."""

    def __init__(self, *shape):
        self.shape = shape
        self.size = int(np.prod(shape))
        self.buf = torch.full((self.size + PAD,), SENTINEL, dtype=torch.float64, device=DEV)
        torch.cuda.synchronize()
        self.ptr = self.buf.data_ptr()

    def get(self):
        a = self.buf.cpu().numpy()
        assert np.all(a[self.size:] == SENTINEL), "the padding behind an output was written"
        return a[:self.size].reshape(self.shape).copy()


def _rows(a, rows):
    """Rows `rows` of an array, of every array of a list, or None."""
    if a is None:
        return None
    return [_rows(x, rows) for x in a] if isinstance(a, (list, tuple)) else a[rows]


def rows_equal_their_own_batch(what, run, *arrays):
    """run(*arrays) on GRID_N problems (arrays, or lists of arrays, with the problem as their first axis; the outputs come back as one flat
    list): GRID_ROWS of every output equal, bit for bit, the same problems run as a batch of their own."""
    full = run(*arrays)
    for rows in GRID_ROWS:
        own = run(*[_rows(a, rows) for a in arrays])
        assert len(own) == len(full)
        for j, (a, b) in enumerate(zip(full, own)):
            assert _same_bits(a[rows], b), (what, rows, "output %d" % j)


def _inputs(orc, kappa, n, seed=41):
    """n problems of all three generators (thirds) with end velocities kappa U(-1, 1) sqrt(L |dX|): end_velocity_gpu_cases._inputs."""
    parts = [er.velocities(orc, d, kappa, n // 3 + 1, seed + d) for d in range(3)]
    return [np.concatenate([p[k] for p in parts])[:n] for k in range(5)]


def _solved_states(n=BIG, variant=rp.VARIANT_F3, dtype=rp.DTYPE_F64, kappa=0.1):
    """(states as the device solve leaves them, the batch still open is not kept): the kappa family, solved on the device."""
    args = _inputs(Oracle(), kappa, n)
    with rp.Batch(n, variant, dtype) as b:
        ts = [_t(a) for a in args]
        b.set_problems_vel_device(*[t.data_ptr() for t in ts])
        b.solve(1e-8, 200, 0)
        return b.get_state()


def _families():
    """name -> spline of BIG problems: solved states with end velocities (a few the solve left with a duration <= 0 are replaced by
    their neighbours: the NaN rule has a case of its own) and random unsolved states."""
    st = _solved_states()
    ok = np.isfinite(st[:, :3]).all(axis=1) & (st[:, 1] > 0) & (st[:, 2] > 0)
    assert ok.mean() > 0.95
    st = st[np.nonzero(ok)[0][np.arange(BIG) % int(ok.sum())]]
    return {"solved": tr.spline_of_state(st), "random": tr.random_states(BIG, 5)}


def _eval(sp, tau, want=(True, True, True)):
    n, k = tau.shape
    ts, tt = [_t(a) for a in sp], _t(tau)
    outs = [Out(n, k) if w else None for w in want]
    capi.trajectory_eval(0, 0, n, k, [t.data_ptr() for t in ts], tt.data_ptr(), *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _vjp(sp, tau, g, want_bars=(True,) * 8, want_tau=True, zero_vel=False):
    """g: three (n, k) arrays or None (a NULL pointer).  Returns (eight bars or None each, tau_bar or None)."""
    n, k = tau.shape
    ts, tt = [_t(a) for a in sp], _t(tau)
    gs = [_t(x) if x is not None else None for x in g]
    bars = [Out(n) if w else None for w in want_bars]
    tb = Out(n, k) if want_tau else None
    addr = [t.data_ptr() for t in ts]
    if zero_vel:
        addr[3] = addr[4] = 0
    capi.trajectory_eval_vjp(0, 0, n, k, addr, tt.data_ptr(), *[x.data_ptr() if x is not None else 0 for x in gs],
                             [o.ptr if o else 0 for o in bars], tb.ptr if tb else 0)
    torch.cuda.synchronize()
    return [o.get() if o else None for o in bars], tb.get() if tb else None


def _jvp(sp, tau, dots, tdot, want=(True, True, True)):
    """dots: eight arrays of n or None each; tdot (n, k) or None."""
    n, k = tau.shape
    ts, tt = [_t(a) for a in sp], _t(tau)
    ds = [_t(x) if x is not None else None for x in dots]
    td = _t(tdot) if tdot is not None else None
    outs = [Out(n, k) if w else None for w in want]
    capi.trajectory_eval_jvp(0, 0, n, k, [t.data_ptr() for t in ts], tt.data_ptr(), [x.data_ptr() if x is not None else 0 for x in ds],
                             td.data_ptr() if td is not None else 0, *[o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _head(sp, n):
    return [a[:n] for a in sp]


def _gradients(n, k, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal((n, k)) for _ in range(3)]


def _tangents(n, k, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n) for _ in range(8)], rng.standard_normal((n, k))


# ---------------------------------------------------------------- 1. forward
def test_forward_against_longdouble_nulls_and_nan_rule():
    fam = _families()
    worst = [0.0, 0.0, 0.0]
    for name, sp_big in fam.items():
        for k in KS:
            tau_big = tr.query_times(sp_big, k, 100 + k)
            for n in NS:
                sp, tau = _head(sp_big, n), tau_big[:n]
                got = _eval(sp, tau)
                want = tr.forward_ld(sp, tau)
                for c, (a, b, scale) in enumerate(zip(got, want, tr.scales(sp))):
                    worst[c] = max(worst[c], float(np.max(np.abs(a - b) / scale)))
                if n == 65 or (n, k) == (BIG, 200):      # every NULL-output combination: the same bits as the full call
                    for combo in itertools.product((False, True), repeat=3):
                        if any(combo):
                            part = _eval(sp, tau, combo)
                            assert all((p is None) == (not w) and (p is None or _same_bits(p, f)) for p, f, w in zip(part, got, combo)), (n, k, combo)
    print("forward against longdouble over %s x %s, both kinds of state: pos %.2e, vel %.2e, acc %.2e of the scale" % (NS, KS, *worst))
    assert max(worst) < 1e-13
    # the NaN rule: a duration <= 0 or inf poisons its problem and no other; a NaN tau its own query and no other
    n, k = 257, 33
    sp = [a.copy() for a in _head(fam["solved"], n)]
    tau = tr.query_times(sp, k, 1)
    clean = _eval(sp, tau)
    sp[6][3], sp[7][64], sp[6][130], sp[7][256] = 0.0, np.inf, -1.0, np.nan
    tau[10, 5] = tau[200, 32] = np.nan
    bad_rows = np.zeros(n, dtype=bool)
    bad_rows[[3, 64, 130, 256]] = True
    bad = np.repeat(bad_rows[:, None], k, axis=1)
    bad[10, 5] = bad[200, 32] = True
    for got, ref in zip(_eval(sp, tau), clean):
        assert np.array_equal(np.isnan(got), bad)
        assert np.array_equal(_bits(got[~bad]), _bits(ref[~bad]))
    bars, tau_bar = _vjp(sp, tau, _gradients(n, k, 2))
    assert np.array_equal(np.isnan(tau_bar), bad)
    for f, b in enumerate(bars):      # a NaN tau is a query of segment 1: its problem's sums over that segment are NaN, pos0_bar and vel0_bar are not
        assert np.isnan(b[bad_rows]).all() and np.isfinite(np.delete(b, [3, 64, 130, 256, 10, 200])).all(), f
        assert np.isnan(b[[10, 200]]).all() == (f not in (0, 3)), f
    for got in _jvp(sp, tau, *_tangents(n, k, 3)):
        assert np.array_equal(np.isnan(got), bad)


# ---------------------------------------------------------------- 2. the batch entry
def test_batch_entry_equals_the_stateless_one_and_the_plot_data():
    orc = Oracle()
    n = 4097
    for variant, dtype, vel in ((rp.VARIANT_F3, rp.DTYPE_F64, True), (rp.VARIANT_F3, rp.DTYPE_F64, False), (rp.VARIANT_F4, rp.DTYPE_F64, True),
                                (rp.VARIANT_F4, rp.DTYPE_F32_STATE, True), (rp.VARIANT_F4, rp.DTYPE_F32_STATE, False)):
        args = _inputs(orc, 0.1, n)
        with rp.Batch(n, variant, dtype) as b:
            ts = [_t(a) for a in args]
            if vel:
                b.set_problems_vel_device(*[t.data_ptr() for t in ts])
            else:
                b.set_problems_device(*[t.data_ptr() for t in ts[:3]])
            b.solve(1e-8, 200, 0)
            slots = b.slot_map()
            assert not np.array_equal(slots, np.arange(n)), "the batch kept problem order: nothing to gather"
            st = b.get_state()
            sp = tr.spline_of_state(st, variant)
            live = np.isfinite(st[:, :3]).all(axis=1) & (st[:, 1] > 0) & (st[:, 2] > 0)
            for k in (1, 33, 64, 200):
                tau = tr.query_times([np.abs(a) for a in sp], k, 7 + k)
                tt = _t(tau)
                outs = [Out(n, k) for _ in range(3)]
                b.trajectory_device(tt.data_ptr(), k, *[o.ptr for o in outs])
                b.sync()
                got = [o.get() for o in outs]
                for g, w in zip(got, _eval(sp, tau)):
                    assert _same_bits(g, w), (variant, dtype, vel, k)
                only_vel = Out(n, k)
                b.trajectory_device(tt.data_ptr(), k, 0, only_vel.ptr, 0)
                b.sync()
                assert _same_bits(only_vel.get(), got[1])
            # at the 33-point grid of each segment: rp_batch_sample's positions and end accelerations
            d0, d1 = sp[6][:, None], sp[7][:, None]
            j = np.arange(33)[None, :]
            tau = np.concatenate([d0 * (j / 32.0), d0 + d1 * (j / 32.0)], axis=1)
            tau[:, 32] = np.nextafter(sp[6], 0.0)
            tt = _t(tau)
            outs = [Out(n, 66), None, Out(n, 66)]
            b.trajectory_device(tt.data_ptr(), 66, outs[0].ptr, 0, outs[2].ptr)
            b.sync()
            pos66, acc4 = b.sample()
            sc = tr.scales(_head([a[live] for a in sp], int(live.sum())))
            e_pos = float(np.max(np.abs(outs[0].get()[live] - pos66[live]) / sc[0]))
            e_acc = float(np.max(np.abs(outs[2].get()[live][:, [0, 32, 33, 65]] - acc4[live]) / sc[2]))
            print("variant %d dtype %d vel %s: %d live problems, against rp_batch_sample pos %.2e acc %.2e of the scale"
                  % (variant, dtype, vel, int(live.sum()), e_pos, e_acc))
            assert live.mean() > 0.9 and e_pos < 1e-13 and e_acc < 1e-13


# ---------------------------------------------------------------- 3. derivatives against longdouble
def test_vjp_and_jvp_against_longdouble():
    """Normwise per problem against the longdouble definition: the float64 restatement of the kernels' arithmetic and order first, on the
    same inputs on the CPU; the device is held to 10 x the restatement's worst (DESIGN.md section 12's margin for a different box and
    different data).  NULL gradient / tangent pointers equal explicit zeros bit for bit."""
    fam = _families()
    worst = {"vjp": [0.0, 0.0], "jvp": [0.0, 0.0]}      # [restatement, device]
    for name, sp_big in fam.items():
        for k in KS:
            tau_big = tr.query_times(sp_big, k, 200 + k)
            g_big = _gradients(BIG, k, 300 + k)
            dots_big, tdot_big = _tangents(BIG, k, 400 + k)
            for n in NS:
                sp, tau = _head(sp_big, n), tau_big[:n]
                g = [x[:n] for x in g_big]
                dots, tdot = [x[:n] for x in dots_big], tdot_big[:n]
                bars_ld, tb_ld = tr.vjp_ld(sp, tau, *g)
                bars_64, tb_64 = tr.vjp_f64(sp, tau, *g)
                bars, tb = _vjp(sp, tau, g)
                worst["vjp"][0] = max(worst["vjp"][0], float(np.max(tr.normwise(bars_64 + [tb_64], bars_ld + [tb_ld]))))
                worst["vjp"][1] = max(worst["vjp"][1], float(np.max(tr.normwise(bars + [tb], bars_ld + [tb_ld]))))
                out_ld = tr.jvp_ld(sp, tau, dots, tdot)
                worst["jvp"][0] = max(worst["jvp"][0], float(np.max(tr.normwise(tr.jvp_f64(sp, tau, dots, tdot), out_ld))))
                worst["jvp"][1] = max(worst["jvp"][1], float(np.max(tr.normwise(_jvp(sp, tau, dots, tdot), out_ld))))
                if n == 65:
                    zero = np.zeros((n, k))
                    for null in itertools.product((False, True), repeat=3):
                        if any(null):
                            a = _vjp(sp, tau, [None if z else x for x, z in zip(g, null)])
                            e = _vjp(sp, tau, [zero if z else x for x, z in zip(g, null)])
                            assert all(_same_bits(x, y) for x, y in zip(a[0] + [a[1]], e[0] + [e[1]])), (k, null)
                    # outputs not asked for change nothing in the others; NULL end velocities are zeros
                    part = _vjp(sp, tau, g, want_bars=(True, False) * 4, want_tau=False)
                    assert part[1] is None and all((p is None) == bool(f % 2) and (p is None or _same_bits(p, bars[f])) for f, p in enumerate(part[0]))
                    sp0 = [a.copy() for a in sp]
                    sp0[3][:] = 0.0
                    sp0[4][:] = 0.0
                    a, e = _vjp(sp0, tau, g, zero_vel=True), _vjp(sp0, tau, g)
                    assert all(_same_bits(x, y) for x, y in zip(a[0] + [a[1]], e[0] + [e[1]]))
                    zn = np.zeros(n)
                    for null in ((True,) * 8 + (False,), (False,) * 8 + (True,), (True, False) * 4 + (True,)):
                        a = _jvp(sp, tau, [None if z else x for x, z in zip(dots, null)], None if null[8] else tdot)
                        e = _jvp(sp, tau, [zn if z else x for x, z in zip(dots, null)], zero if null[8] else tdot)
                        assert all(_same_bits(x, y) for x, y in zip(a, e)), (k, null)
    for what, (restated, device) in worst.items():
        print("%s against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (what, restated, device, 10 * restated))
        assert device <= 10 * restated, what


# ---------------------------------------------------------------- 4. reproducibility
def test_bits_do_not_depend_on_the_batch_or_the_run():
    fam = _families()
    for name, sp_big in fam.items():
        for k in KS:
            tau_big = tr.query_times(sp_big, k, 500 + k)
            g_big = _gradients(BIG, k, 600 + k)
            dots_big, tdot_big = _tangents(BIG, k, 700 + k)
            fwd = _eval(sp_big, tau_big)
            bars, tb = _vjp(sp_big, tau_big, g_big)
            again = _vjp(sp_big, tau_big, g_big)
            assert all(_same_bits(x, y) for x, y in zip(bars + [tb], again[0] + [again[1]])), "the VJP differs from run to run"
            fwd_dot = _jvp(sp_big, tau_big, dots_big, tdot_big)
            for n in NS[:-1]:
                sp, tau = _head(sp_big, n), tau_big[:n]
                for a, b in zip(_eval(sp, tau), fwd):
                    assert _same_bits(a, b[:n]), (name, n, k)
                small = _vjp(sp, tau, [x[:n] for x in g_big])
                for a, b in zip(small[0] + [small[1]], bars + [tb]):
                    assert _same_bits(a, b[:n]), (name, n, k)
                for a, b in zip(_jvp(sp, tau, [x[:n] for x in dots_big], tdot_big[:n]), fwd_dot):
                    assert _same_bits(a, b[:n]), (name, n, k)
            # ... nor on where in a batch the problem sits: problem 0 again as the last of 4097
            moved = [np.concatenate([a[1:], a[:1]]) for a in sp_big]
            roll = lambda x: np.concatenate([x[1:], x[:1]])      # noqa: E731
            m = _vjp(moved, roll(tau_big), [roll(x) for x in g_big])
            for a, b in zip(m[0] + [m[1]], bars + [tb]):
                assert _same_bits(a[-1], b[0]) and _same_bits(a[:-1], b[1:]), (name, k)
    # ... nor on which of a block's trips the problem is in: more trips than the grid's cap
    sp = tr.random_states(GRID_N, 77)
    for k in GRID_KS:
        tau = tr.query_times(sp, k, 800 + k)
        dots, tdot = _tangents(GRID_N, k, 820 + k)
        rows_equal_their_own_batch(("eval", k), _eval, sp, tau)
        rows_equal_their_own_batch(("vjp", k), lambda s, t, g: (lambda r: r[0] + [r[1]])(_vjp(s, t, g)), sp, tau, _gradients(GRID_N, k, 810 + k))
        rows_equal_their_own_batch(("jvp", k), _jvp, sp, tau, dots, tdot)


# ---------------------------------------------------------------- 5. autograd
def test_autograd_reverse_forward_and_duality():
    fam = _families()
    n, k = 257, 33
    for name, sp_big in fam.items():
        sp = _head(sp_big, n)
        tau = tr.query_times(sp, k, 8, exact=False, keep_off_knot=1e-3)
        g = [_t(x) for x in _gradients(n, k, 9)]
        names = ("pos0", "pos1", "pos2", "vel0", "vel2", "vel1", "duration0", "duration1")
        ins = {nm: _t(a).requires_grad_() for nm, a in zip(names, sp)}
        t = _t(tau).requires_grad_()

        def run(v, tt):
            return rp.trajectory_eval(v["pos0"], v["pos1"], v["pos2"], v["vel1"], v["duration0"], v["duration1"], tt, vel0=v["vel0"], vel2=v["vel2"])

        def loss_rows(v, tt):
            return sum(gi * o for gi, o in zip(g, run(v, tt)))

        grads = torch.autograd.grad(loss_rows(ins, t).sum(), [ins[nm] for nm in names] + [t])
        # central differences of the device op, step 1e-6 max(|x|, 1): truncation ~1e-12 x third derivatives, rounding ~1e-16 / 1e-6
        fd = []
        with torch.no_grad():
            for nm in names:
                h = 1e-6 * ins[nm].abs().clamp(min=1.0)
                up, dn = dict(ins), dict(ins)
                up[nm], dn[nm] = ins[nm] + h, ins[nm] - h
                fd.append(((loss_rows(up, t) - loss_rows(dn, t)).sum(1) / (2 * h)).cpu().numpy())
            h = 1e-6 * t.abs().clamp(min=1.0)
            fd_tau = ((loss_rows(ins, t + h) - loss_rows(ins, t - h)) / (2 * h)).cpu().numpy()
        e_par = float(np.max(tr.normwise([x.cpu().numpy() for x in grads[:8]], fd)))
        e_tau = float(np.max(tr.normwise([grads[8].cpu().numpy()], [fd_tau])))
        print("%s: reverse mode against central differences of the device op, normwise: spline inputs %.2e, tau %.2e" % (name, e_par, e_tau))
        assert e_par < 1e-6 and e_tau < 1e-6
        # a (k,) tau is every problem's tau; only the inputs that ask get a gradient; vel0 / vel2 of None are zeros
        row = _t(tau[0]).requires_grad_()
        o = rp.trajectory_eval(*[ins[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")], row)
        z = np.zeros(n)
        w = _eval([sp[0], sp[1], sp[2], z, z, sp[5], sp[6], sp[7]], np.repeat(tau[:1], n, axis=0))
        assert all(_same_bits(a.detach().cpu().numpy(), b) for a, b in zip(o, w))
        (g_row,) = torch.autograd.grad(o[0].sum(), row)
        assert g_row.shape == (k,)
        # a loss on pos alone: the gradients of the two outputs it does not use reach the kernel as NULL
        only = torch.autograd.grad((g[0] * run(ins, t)[0]).sum(), [ins[nm] for nm in names] + [t])
        w_bars, w_tau = _vjp(sp, tau, [g[0].cpu().numpy(), None, None])
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(only, w_bars + [w_tau])), name
        # forward mode: forward_ad and torch.func.jvp are the JVP entry
        dots, tdot = _tangents(n, k, 10)
        want = _jvp(sp, tau, dots, tdot)
        with fwAD.dual_level():
            dual = {nm: fwAD.make_dual(ins[nm].detach(), _t(d)) for nm, d in zip(names, dots)}
            outs = run(dual, fwAD.make_dual(t.detach(), _t(tdot)))
            got = [fwAD.unpack_dual(x).tangent.cpu().numpy() for x in outs]
        assert all(_same_bits(a, b) for a, b in zip(got, want)), name

        def f(*xs):
            return run(dict(zip(names, xs[:8])), xs[8])
        _, got = torch.func.jvp(f, tuple(ins[nm].detach() for nm in names) + (t.detach(),), tuple(_t(d) for d in dots) + (_t(tdot),))
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(got, want)), name
        # duality between the two modes: <g, J u> = <J^T g, u>, each side a float64 sum of terms that carry the kernels' ~1e-15
        left = sum(float((gi.cpu().numpy().astype(np.longdouble) * o).sum()) for gi, o in zip(g, want))
        terms = [gr.cpu().numpy().astype(np.longdouble) * d for gr, d in zip(grads[:8], dots)] + [grads[8].cpu().numpy().astype(np.longdouble) * tdot]
        right = sum(float(x.sum()) for x in terms)
        size = sum(float(np.abs(x).sum()) for x in terms) + sum(float(np.abs(gi.cpu().numpy() * o).sum()) for gi, o in zip(g, want))
        # bound: both sides hold to the 10 x 3e-15 normwise of the check against longdouble; by Cauchy-Schwarz their sums differ by at most
        # that times |g| |J u| + |J^T g| |u|, which for these random directions is a few times the sum of |terms|: 1e-12
        print("%s: duality between reverse and forward mode: %.2e of the sum of |terms|" % (name, abs(left - right) / size))
        assert abs(left - right) <= 1e-12 * size
        # first order only
        (g0,) = torch.autograd.grad((run(ins, t)[0] ** 2).sum(), ins["vel1"], create_graph=True)
        try:
            g0.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("double backward did not raise")
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. end to end
def test_min_time_trajectory_against_differences_of_the_pipeline():
    orc = Oracle()
    n, k = 4096, 8
    args = _inputs(orc, 0.1, n)
    names = ("pos0", "pos1", "pos2", "vel0", "vel2")
    x = {nm: _t(a).requires_grad_() for nm, a in zip(names, args)}
    with torch.no_grad():
        first = rp.min_time_solve(x["pos0"], x["pos1"], x["pos2"], vel0=x["vel0"], vel2=x["vel2"], gap_tol=1e-13)
    d0, d1 = first[1].cpu().numpy(), first[2].cpu().numpy()
    usable = np.isfinite(d0) & np.isfinite(d1) & (d0 > 0) & (d1 > 0)
    spl = [None] * 6 + [np.where(usable, d0, 1.0), np.where(usable, d1, 1.0)]
    tau = _t(tr.query_times(spl, k, 21, exact=False, keep_off_knot=1e-3)).requires_grad_()      # fixed times: no part of the solution
    rng = np.random.default_rng(22)
    wp, wv = _t(rng.uniform(0.5, 1.5, (n, k))), _t(rng.uniform(0.5, 1.5, (n, k)) * 0.1)

    def rows(v, tt):
        out = rp.min_time_trajectory(v["pos0"], v["pos1"], v["pos2"], tt, vel0=v["vel0"], vel2=v["vel2"], gap_tol=1e-13)
        return wp * out[0] + wv * out[1], out[7]

    loss, status = rows(x, tau)
    grads = torch.autograd.grad(loss.sum(), [x[nm] for nm in names] + [tau])
    ok = ((status & capi.ST_CONVERGED) != 0) & torch.isfinite(torch.stack(grads[:5], 1)).all(1) & torch.isfinite(grads[5]).all(1) & _t(usable).bool()
    h = 1e-4
    stats = []
    with torch.no_grad():
        for i, nm in enumerate(names):
            up, dn = dict(x), dict(x)
            up[nm], dn[nm] = x[nm] + h, x[nm] - h
            fd = (rows(up, tau)[0] - rows(dn, tau)[0]).sum(1) / (2 * h)
            stats.append((nm, ((grads[i] - fd).abs() / fd.abs().clamp(min=1e-3))[ok]))
        fd = (rows(x, tau + h)[0] - rows(x, tau - h)[0]) / (2 * h)
        stats.append(("tau", ((grads[5] - fd).abs() / fd.abs().clamp(min=1e-3))[ok].reshape(-1)))
    print("%d of %d problems converged and finite" % (int(ok.sum()), n))
    for nm, rel in stats:
        print("  d / d %-5s against central differences of the pipeline: median %.2e, 95 %% %.2e" % (nm, rel.median(), rel.quantile(0.95)))
    assert ok.float().mean() > 0.95
    for nm, rel in stats:
        assert rel.median() < 1e-5 and rel.quantile(0.95) < 1e-3, nm
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 7. identities
def test_end_point_identities_with_normalized_time():
    orc = Oracle()
    n = 4096
    args = _inputs(orc, 0.1, n)
    names = ("pos0", "pos1", "pos2", "vel0", "vel2")
    x = {nm: _t(a).requires_grad_() for nm, a in zip(names, args)}
    u = torch.tensor([0.0, 1.0], dtype=torch.float64, device=DEV)
    out = rp.min_time_trajectory(x["pos0"], x["pos1"], x["pos2"], u, normalized=True, vel0=x["vel0"], vel2=x["vel2"], gap_tol=1e-13)
    pos, vel, _, vel1, d0, d1, _, status = out
    sol = [t.detach().cpu().numpy() for t in (vel1, d0, d1)]
    live = np.isfinite(np.stack(sol, 1)).all(1) & (sol[1] > 0) & (sol[2] > 0)
    sp = [args[0], args[1], args[2], args[3], args[4]] + sol
    sc = tr.scales([np.where(live, a, 1.0) for a in sp])
    p, v = pos.detach().cpu().numpy(), vel.detach().cpu().numpy()
    e = [np.abs(p[:, 0] - args[0]) / sc[0][:, 0], np.abs(p[:, 1] - args[2]) / sc[0][:, 0], np.abs(v[:, 1] - args[4]) / sc[1][:, 0]]
    print("pos(0) = pos0 %.2e, pos(1) = pos2 %.2e, vel(1) = vel2 %.2e of the scale, on %d live problems" % (*[float(x[live].max()) for x in e], int(live.sum())))
    assert live.mean() > 0.95 and all(float(x[live].max()) < 1e-12 for x in e)
    # the total derivatives: d pos(u = 1) / d (pos0, pos1, pos2, vel0, vel2) = (0, 0, 1, 0, 0), d pos(u = 0) / d ... = (1, 0, 0, 0, 0), within
    # 1e-10 of the largest term of each chain-rule sum -- the terms: the evaluator's own gradients, and its gradients in (vel1, duration0,
    # duration1) and tau times the solve's Jacobian
    jac = rp.min_time_jacobian(*[x[nm].detach() for nm in names[:3]], vel0=x["vel0"].detach(), vel2=x["vel2"].detach(), gap_tol=1e-13)[5].cpu().numpy()
    fine = live & np.isfinite(jac.reshape(n, -1)).all(1) & ((status.cpu().numpy() & capi.ST_CONVERGED) != 0)
    assert fine.mean() > 0.95
    T = sol[1] + sol[2]
    tau = np.stack([np.zeros(n), T], axis=1)
    for col, expected in ((1, (0.0, 0.0, 1.0, 0.0, 0.0)), (0, (1.0, 0.0, 0.0, 0.0, 0.0))):
        total = torch.autograd.grad(pos[:, col].sum(), [x[nm] for nm in names], retain_graph=True)
        total = np.stack([t.cpu().numpy() for t in total], 1)
        g = np.zeros((n, 2))
        g[:, col] = 1.0
        live_sp = [np.where(fine, a, 1.0) for a in sp]
        bars, tau_bar = _vjp(live_sp, np.where(fine[:, None], tau, 0.5), [g, None, None])
        through_tau = tau_bar[:, col] * float(col)      # tau = u (duration0 + duration1): d tau / d duration = u
        direct = np.stack([bars[0], bars[1], bars[2], bars[3], bars[4]], 1)
        worst = 0.0
        for bcol in range(5):
            terms = np.stack([direct[:, bcol], bars[5] * jac[:, 0, bcol], bars[6] * jac[:, 1, bcol], bars[7] * jac[:, 2, bcol],
                              through_tau * jac[:, 1, bcol], through_tau * jac[:, 2, bcol], np.full(n, expected[bcol])], 1)
            largest = np.abs(terms).max(1)
            miss = np.abs(total[:, bcol] - expected[bcol]) / np.maximum(largest, 1e-300)
            worst = max(worst, float(miss[fine].max()))
        print("d pos(u = %d) / d (pos0, pos1, pos2, vel0, vel2): off by %.2e of the largest chain-rule term" % (col, worst))
        assert worst < 1e-10
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]]()
    print("case ok")
