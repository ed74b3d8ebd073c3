"""The cases of tests/test_gpu_integrals.py, each run in a fresh process (`python tests/integrals_gpu_cases.py <case> [family]`), on top of
tests/trajectory_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is checked, and why each bound is
what it is: DESIGN.md section 16."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import trajectory_gpu_cases as tg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import crossing_ref as cr  # noqa: E402
import extrema_ref as xr  # noqa: E402
import integrals_ref as ir  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from oracle_api import Oracle  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

DEV, BIG = tg.DEV, tg.BIG
KS = (1, 2, 7, 8)                    # odd k and odd totals (BIG is odd) take the unpaired path of stream_pairs
VJP_KS = KS + (33, 64, 65, 200)      # every group size G, both pair paths, more units than lanes
LD = np.longdouble
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
    """extrema_ref.windows with, from the fourth column on, every other column a short window (integrals_ref.short_windows); the knot
    family has its own window in every column."""
    if name == "knot":
        _, lo, hi, _ = xr.knot_cases()
        return np.repeat(lo, k, axis=1), np.repeat(hi, k, axis=1)
    lo, hi = xr.windows(sp, k, seed)
    slo, shi = ir.short_windows(sp, k, seed + 1)
    lo[:, 3::2], hi[:, 3::2] = slo[:, 3::2], shi[:, 3::2]
    return lo, hi


def _addr(sp, zero_vel=False):
    """(the spline's eight device tensors -- the caller holds them while the launch runs --, their addresses)"""
    ts = [_t(a) for a in sp]
    addr = [t.data_ptr() for t in ts]
    if zero_vel:
        addr[3] = addr[4] = 0
    return ts, addr


def _dev(a):
    return _t(a) if a is not None else None


def _ptr(t):
    return t.data_ptr() if t is not None else 0


def _int(sp, lo, hi, k=None, want=ALL, zero_vel=False):
    """The stateless entry: four arrays, None where not asked for.  lo / hi of None go in as NULL."""
    n = len(sp[0])
    k = k if k is not None else (lo if lo is not None else hi).shape[1]
    ts, addr = _addr(sp, zero_vel)
    tl, th = _dev(lo), _dev(hi)
    outs = [Out(n, k) if w else None for w in want]
    capi.trajectory_integrals(0, 0, n, k, addr, _ptr(tl), _ptr(th), [o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _ivjp(sp, lo, hi, g, want_bars=(True,) * 8, want_lo=True, want_hi=True, k=None):
    """g: four (n, k) arrays or None each (NULL), or None (a NULL table).  Returns (eight bars or None each, lo_bar, hi_bar)."""
    n = len(sp[0])
    k = k if k is not None else (lo if lo is not None else hi).shape[1]
    ts, addr = _addr(sp)
    tl, th = _dev(lo), _dev(hi)
    gs = [_dev(x) for x in g] if g is not None else None
    bars = [Out(n) if w else None for w in want_bars]
    lb, hb = Out(n, k) if want_lo else None, Out(n, k) if want_hi else None
    capi.trajectory_integrals_vjp(0, 0, n, k, addr, _ptr(tl), _ptr(th), [_ptr(x) for x in gs] if gs is not None else None,
                                  [o.ptr if o else 0 for o in bars], lb.ptr if lb else 0, hb.ptr if hb else 0)
    torch.cuda.synchronize()
    return [o.get() if o else None for o in bars], lb.get() if lb else None, hb.get() if hb else None


def _ijvp(sp, lo, hi, dots, lo_dot, hi_dot, want=ALL, k=None):
    """dots: eight arrays of n or None each, or None (a NULL table); lo_dot, hi_dot (n, k) or None."""
    n = len(sp[0])
    k = k if k is not None else (lo if lo is not None else hi).shape[1]
    ts, addr = _addr(sp)
    tl, th, tld, thd = _dev(lo), _dev(hi), _dev(lo_dot), _dev(hi_dot)
    ds = [_dev(x) for x in dots] if dots is not None else None
    outs = [Out(n, k) if w else None for w in want]
    capi.trajectory_integrals_jvp(0, 0, n, k, addr, _ptr(tl), _ptr(th), [_ptr(x) for x in ds] if ds is not None else None, _ptr(tld), _ptr(thd),
                                  [o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _all_same(a, b):
    return all(_same_bits(x, y) for x, y in zip(a, b))


def _flat(v):
    """(bars, lo_bar, hi_bar) as one list of ten."""
    return list(v[0]) + [v[1], v[2]]


def _of_scale(sp, lo, hi, got, want):
    """Per output the worst |got - want| / (scale x (b - a)) over the queries with a < b."""
    a, b, ok = ir.clamped(sp, lo, hi)
    with np.errstate(all="ignore"):
        live = ok & (b > a)
        W = np.where(live, b - a, LD(1))
        return [float(np.where(live, np.abs(np.asarray(g, dtype=LD) - w) / (s * W), 0).max()) for g, w, s in zip(got, want, ir.value_scales(sp))]


# ---------------------------------------------------------------- 1. forward
def test_forward_against_the_definition(family):
    sp = _family(family)
    n = len(sp[0])
    device, restated = 0.0, 0.0
    for k in KS:
        lo, hi = _windows(family, sp, k, 300 + k)
        want = ir.integrals_ld(sp, lo, hi)
        f64 = ir.integrals_f64(sp, lo, hi)
        got = _int(sp, lo, hi)
        a, b, ok = ir.clamped(sp, lo, hi)
        for j, name in enumerate(ir.NAMES):
            assert np.array_equal(np.isnan(got[j]), np.isnan(want[j])), (family, k, name, "the NaN mask")
            same = ok & (a == b)
            assert np.all(got[j][same] == 0) and not np.signbit(got[j][same]).any(), (family, k, name, "a == b")
        device = max(device, max(_of_scale(sp, lo, hi, got, want)))
        restated = max(restated, max(_of_scale(sp, lo, hi, f64, want)))
        # a NULL window end is the infinite one, bit for bit (column 0 has both)
        inf = np.full(lo.shape, np.inf)
        assert _all_same(_int(sp, None, hi), _int(sp, -inf, hi)) and _all_same(_int(sp, lo, None), _int(sp, lo, inf)), (family, k)
        assert _all_same(_int(sp, None, None, k=k), _int(sp, -inf, inf)), (family, k)
        if k == 7:
            # every output alone, and every output alone left out: the others' bits do not change, and nothing else is written
            for f in range(4):
                for alone in (True, False):
                    wanted = [(g == f) == alone for g in range(4)]
                    some = _int(sp, lo, hi, want=wanted)
                    for g, x in enumerate(some):
                        assert (x is None) == (not wanted[g]) and (x is None or _same_bits(x, got[g])), (family, f, alone, g)
    print("%s (%d problems) x %s: values against the definition, of scale x (b - a): the device %.3g, the float64 restatement %.3g, asserted %.3g"
          % (family, n, KS, device, restated, 10 * restated))
    assert device <= 10 * restated, family      # ten times what the float64 restatement holds on the same inputs (section 12's margin)
    if family == "knot":
        # the known answer is its problem 0 over the whole spline
        whole = _int(_head(sp, 1), None, None, k=1)
        for x, w in zip(whole, (100.0, 200.0, 24000.0, 240000.0)):
            assert abs(x[0, 0] - w) <= 1e-13 * w, (x[0, 0], w)
        return
    # the NaN rule: a duration of 0, -1, inf, NaN poisons its problem and no other; a NaN window end its own query and no other
    m, k = 257, 7
    sp = [a.copy() for a in _head(sp, m)]
    lo, hi = xr.windows(sp, k, 1)
    clean = _int(sp, lo, hi)
    sp[6][3], sp[7][64], sp[6][130], sp[7][256] = 0.0, np.inf, -1.0, np.nan
    lo[10, 0], hi[200, 4], lo[11, 3], hi[11, 3] = np.nan, np.nan, np.inf, np.inf
    bad = np.zeros((m, k), dtype=bool)
    bad[[3, 64, 130, 256]] = True
    bad[10, 0] = bad[200, 4] = bad[11, 3] = True
    for x, ref in zip(_int(sp, lo, hi), clean):
        assert np.array_equal(np.isnan(x), bad | np.isnan(ref)), family
        assert np.array_equal(_bits(x[~bad]), _bits(ref[~bad])), family
    if family == "rest":      # NULL end velocities are zeros
        head = _head(_family(family), 65)
        assert _all_same(_int(head, lo[:65], hi[:65], zero_vel=True), _int(head, lo[:65], hi[:65]))


# ---------------------------------------------------------------- 2. the batch entry
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
                    outs = [Out(n, k) for _ in range(4)]
                    b.integrals_device(tl.data_ptr(), th.data_ptr(), k, [o.ptr for o in outs])
                    b.sync()
                    got = [o.get() for o in outs]
                    assert _all_same(got, _int(sp, lo, hi)), (variant, dtype, vel, k)
                    only = Out(n, k)
                    b.integrals_device(0, 0, k, [0, only.ptr, 0, 0])      # the whole spline's distance travelled, nothing else
                    b.sync()
                    assert _same_bits(only.get(), _int(sp, None, None, k=k)[1])
                finite = float((~np.isnan(got[0])).mean())
                print("variant %d dtype %d vel %s: the batch entry's bits are the stateless entry's; %.1f %% of the windows not empty" % (variant, dtype, vel, 100 * finite))
                assert finite > 0.9


# ---------------------------------------------------------------- 3. both derivative modes
def _zap(xs):
    return [np.where(np.isnan(np.asarray(x, dtype=np.float64)), 0, x) for x in xs]


def test_vjp_and_jvp_against_longdouble(family):
    sp = _family(family)
    n = len(sp[0])
    worst = {"vjp": [0.0, 0.0], "jvp": [0.0, 0.0]}      # (the device, the float64 restatement), normwise per problem against longdouble
    for k in (VJP_KS if family == "random" else KS):
        lo, hi = _windows(family, sp, k, 600 + k)
        rng = np.random.default_rng(700 + k)
        g = [rng.standard_normal((n, k)) for _ in range(4)]
        want = _flat(ir.vjp_ld(sp, lo, hi, g))
        got = _flat(_ivjp(sp, lo, hi, g))
        worst["vjp"][0] = max(worst["vjp"][0], float(np.max(tr.normwise(got, want))))
        worst["vjp"][1] = max(worst["vjp"][1], float(np.max(tr.normwise(_flat(ir.vjp_f64(sp, lo, hi, g)), want))))
        if k in KS:
            dots, lo_dot = tg._tangents(n, k, 800 + k)
            hi_dot = rng.standard_normal((n, k))
            want_dot = ir.jvp_ld(sp, lo, hi, dots, lo_dot, hi_dot)
            got_dot = _ijvp(sp, lo, hi, dots, lo_dot, hi_dot)
            for j in range(4):
                assert np.array_equal(np.isnan(got_dot[j]), np.isnan(want_dot[j])), (family, k, ir.NAMES[j])
            worst["jvp"][0] = max(worst["jvp"][0], float(np.max(tr.normwise(_zap(got_dot), _zap(want_dot)))))
            worst["jvp"][1] = max(worst["jvp"][1], float(np.max(tr.normwise(_zap(ir.jvp_f64(sp, lo, hi, dots, lo_dot, hi_dot)), _zap(want_dot)))))
        if k in (7, 8):      # both pair paths
            # NULL gradients are zeros, bit for bit; a NULL table too
            z = np.zeros((n, k))
            assert _all_same(_flat(_ivjp(sp, lo, hi, [g[0], None, g[2], None])), _flat(_ivjp(sp, lo, hi, [g[0], z, g[2], z]))), (family, k)
            assert _all_same(_flat(_ivjp(sp, lo, hi, None)), _flat(_ivjp(sp, lo, hi, [z, z, z, z]))), (family, k)
            some = [d if f % 2 else None for f, d in enumerate(dots)]
            full = [d if d is not None else np.zeros(n) for d in some]
            assert _all_same(_ijvp(sp, lo, hi, some, None, hi_dot), _ijvp(sp, lo, hi, full, z, hi_dot)), (family, k)
            assert _all_same(_ijvp(sp, lo, hi, None, lo_dot, None), _ijvp(sp, lo, hi, [np.zeros(n)] * 8, lo_dot, z)), (family, k)
            # only the outputs asked for are written (the sentinels behind each are checked by Out.get), with the same bits
            for f in range(10):
                for alone in (True, False):
                    wanted = [(j == f) == alone for j in range(10)]
                    some = _flat(_ivjp(sp, lo, hi, g, want_bars=wanted[:8], want_lo=wanted[8], want_hi=wanted[9]))
                    for j, x in enumerate(some):
                        assert (x is None) == (not wanted[j]) and (x is None or _same_bits(x, got[j])), (family, k, f, alone, j)
            for f in range(4):
                wanted = [j == f for j in range(4)]
                some = _ijvp(sp, lo, hi, dots, lo_dot, hi_dot, want=wanted)
                assert all((x is None) == (not w) and (x is None or _same_bits(x, y)) for x, w, y in zip(some, wanted, got_dot)), (family, k, f)
    for mode, (device, restated) in worst.items():
        print("%s: %s against longdouble, normwise: the device %.2e, the float64 restatement %.2e, asserted %.2e" % (family, mode, device, restated, 10 * restated))
        assert device <= 10 * restated, (family, mode)


# ---------------------------------------------------------------- 4. reproducibility
def test_bits_depend_on_the_problem_and_its_windows_only():
    roll = lambda x: np.concatenate([x[1:], x[:1]])      # noqa: E731
    for family in ("solved", "random", "rest"):
        sp = _family(family)
        for k in (VJP_KS if family == "random" else KS):
            lo, hi = _windows(family, sp, k, 500 + k)
            rng = np.random.default_rng(900 + k)
            g = [rng.standard_normal((BIG, k)) for _ in range(4)]
            dots, lo_dot = tg._tangents(BIG, k, 901 + k)
            hi_dot = rng.standard_normal((BIG, k))
            runs = {"forward": lambda s, a, b, rows: _int(s, a, b),
                    "vjp": lambda s, a, b, rows: _flat(_ivjp(s, a, b, [x[rows] for x in g])),
                    "jvp": lambda s, a, b, rows: _ijvp(s, a, b, [d[rows] for d in dots], lo_dot[rows], hi_dot[rows])}
            if k not in KS:
                runs = {"vjp": runs["vjp"]}
            every = np.arange(BIG)
            for what, run in runs.items():
                first = run(sp, lo, hi, every)
                assert _all_same(first, run(sp, lo, hi, every)), (family, k, what, "differs from run to run")
                for n in (1, 63, 64, 65, 255, 257):
                    assert _all_same(run(_head(sp, n), lo[:n], hi[:n], every[:n]), [x[:n] for x in first]), (family, n, k, what)
                moved = run([roll(a) for a in sp], roll(lo), roll(hi), roll(every))      # problem 0 moved to the end
                for a, b in zip(moved, first):
                    assert _same_bits(a[-1], b[0]) and _same_bits(a[:-1], b[1:]), (family, k, what)
    # more trips than the grid's cap: 300,001 problems of one window each are 2,344 trips of 128 for 2,048 blocks
    n = 300001
    sp = tr.random_states(n, 77)
    lo, hi = (x[:, 2:3].copy() for x in xr.windows(sp, 3, 78))
    got = _int(sp, lo, hi)
    f64 = ir.integrals_f64(sp, lo, hi)
    a, b, ok = ir.clamped(sp, lo, hi, np.float64)
    W = np.where(ok & (b > a), b - a, 1.0)
    worst = 0.0
    for j, scale in enumerate(ir.value_scales(sp)):
        missing = np.isnan(f64[j])
        assert np.array_equal(np.isnan(got[j]), missing), ir.NAMES[j]
        worst = max(worst, float(np.where(missing, 0, np.abs(got[j] - f64[j]) / (scale * W)).max()))
    print("%d problems x 1 window: %.2f %% empty, values within %.2e of scale x (b - a) of the float64 restatement" % (n, 100 * missing.mean(), worst))
    assert 0.002 < missing.mean() < 0.03 and worst <= 1e-12      # section 16's bound on the float64 arithmetic itself
    # the derivatives there: the rows at the start, where the blocks begin their second trip and at the end are those of a batch of their own
    for k in tg.GRID_KS:
        lo, hi = xr.windows(sp, k, 800 + k)
        rng = np.random.default_rng(810 + k)
        g = [rng.standard_normal((n, k)) for _ in range(4)]
        dots, lo_dot = tg._tangents(n, k, 820 + k)
        tg.rows_equal_their_own_batch(("integrals vjp", k), lambda s, a, b, gg: _flat(_ivjp(s, a, b, gg)), sp, lo, hi, g)
        tg.rows_equal_their_own_batch(("integrals jvp", k), _ijvp, sp, lo, hi, dots, lo_dot, rng.standard_normal((n, k)))


# ---------------------------------------------------------------- 5. autograd
def test_autograd_reverse_forward_and_duality():
    n, k = BIG, 7
    for family in ("solved", "random", "rest"):
        sp = _family(family)
        lo_np, hi_np = xr.windows(sp, k, 8)
        ins = {nm: _t(a).requires_grad_() for nm, a in zip(NAMES, sp)}
        lo, hi = _t(lo_np).requires_grad_(), _t(hi_np).requires_grad_()
        rng = np.random.default_rng(9)
        gn = [rng.standard_normal((n, k)) for _ in range(4)]
        g = [_t(x) for x in gn]

        def run(v, a, b):
            return rp.trajectory_integrals(v["pos0"], v["pos1"], v["pos2"], v["vel1"], v["duration0"], v["duration1"], a, b, vel0=v["vel0"], vel2=v["vel2"])

        outs = run(ins, lo, hi)
        assert len(outs) == 4 and all(o.requires_grad and o.shape == (n, k) for o in outs)
        dev = _int(sp, lo_np, hi_np)
        assert all(_same_bits(o.detach().cpu().numpy(), x) for o, x in zip(outs, dev)), family
        leaves = [ins[nm] for nm in NAMES] + [lo, hi]
        got = [x.cpu().numpy() for x in torch.autograd.grad(outs, leaves, grad_outputs=g, retain_graph=True)]
        hand = _flat(_ivjp(sp, lo_np, hi_np, gn))
        assert _all_same(got, hand), family
        miss = np.isnan(dev[0])
        assert miss.any() and all(np.isfinite(x).all() for x in got) and np.all(got[8][miss] == 0) and np.all(got[9][miss] == 0), family
        # a NaN output's gradient is exactly 0: upstream gradients on the NaN outputs alone reach nothing
        only = [torch.where(_t(miss).bool(), x, torch.zeros_like(x)) for x in g]
        assert all(np.all(x.cpu().numpy() == 0) for x in torch.autograd.grad(outs, leaves, grad_outputs=only, retain_graph=True)), family
        # an output the loss does not use costs nothing and changes nothing
        part = [x.cpu().numpy() for x in torch.autograd.grad([outs[1], outs[3]], leaves, grad_outputs=[g[1], g[3]], retain_graph=True)]
        assert _all_same(part, _flat(_ivjp(sp, lo_np, hi_np, [None, gn[1], None, gn[3]]))), family
        # only the gradients autograd needs are formed
        (one,) = torch.autograd.grad(outs, [lo], grad_outputs=g, retain_graph=True)
        assert _same_bits(one.cpu().numpy(), hand[8]), family
        # forward mode
        dots_np, lo_dot_np = tg._tangents(n, k, 10)
        hi_dot_np = rng.standard_normal((n, k))
        dots, lo_dot, hi_dot = [_t(d) for d in dots_np], _t(lo_dot_np), _t(hi_dot_np)
        want_dot = _ijvp(sp, lo_np, hi_np, dots_np, lo_dot_np, hi_dot_np)
        with fwAD.dual_level():
            dual = {nm: fwAD.make_dual(ins[nm].detach(), d) for nm, d in zip(NAMES, dots)}
            douts = run(dual, fwAD.make_dual(lo.detach(), lo_dot), fwAD.make_dual(hi.detach(), hi_dot))
            got_dot = [fwAD.unpack_dual(o).tangent.cpu().numpy() for o in douts]
        assert _all_same(got_dot, want_dot), family

        def f(*xs):
            return run(dict(zip(NAMES, xs[:8])), xs[8], xs[9])
        _, func_dot = torch.func.jvp(f, tuple(x.detach() for x in leaves), tuple(dots) + (lo_dot, hi_dot))
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(func_dot, want_dot)), family
        # duality between the two modes: <g, J u> = <J^T g, u>
        left_terms = [np.where(np.isnan(d), 0, x.astype(LD) * d) for x, d in zip(gn, got_dot)]
        right_terms = [x.astype(LD) * d for x, d in zip(got[:8], dots_np)] + [got[8].astype(LD) * lo_dot_np, got[9].astype(LD) * hi_dot_np]
        left, right = sum(float(x.sum()) for x in left_terms), sum(float(x.sum()) for x in right_terms)
        size = sum(float(np.abs(x).sum()) for x in left_terms + right_terms)
        print("%s: duality between reverse and forward mode: %.2e of the sum of |terms|" % (family, abs(left - right) / size))
        assert abs(left - right) <= 1e-12 * size, family
        # first order only
        (g0,) = torch.autograd.grad((torch.nan_to_num(run(ins, lo, hi)[2]) ** 2).sum(), ins["vel1"], create_graph=True)
        try:
            g0.sum().backward()
        except RuntimeError as e:
            assert "once_differentiable" in str(e), e
        else:
            raise AssertionError("double backward did not raise")
        # reverse mode against central differences of the device op, on the queries the CPU rule keeps
        keep_np = ir.kept_for_differences(sp, lo_np, hi_np)
        keep = _t(keep_np).bool()
        share = keep_np.sum() / (~miss)[:, [0] + list(range(2, k))].sum()
        gk = [torch.where(keep, x, torch.zeros_like(x)) for x in g]
        grads = [x.cpu().numpy() for x in torch.autograd.grad(outs, leaves, grad_outputs=gk, retain_graph=True)]

        def loss(v, a, b):
            with torch.no_grad():
                return sum(torch.where(keep, x * o, torch.zeros_like(o)) for x, o in zip(gk, run(v, a, b)))

        fd = []
        for nm in NAMES:
            h = 1e-6 * ins[nm].detach().abs().clamp(min=1.0)
            up, dn = dict(ins), dict(ins)
            up[nm], dn[nm] = ins[nm].detach() + h, ins[nm].detach() - h
            fd.append(((loss(up, lo, hi).sum(1) - loss(dn, lo, hi).sum(1)) / (2 * h)).cpu().numpy())
        for which in (0, 1):
            x = (lo, hi)[which].detach()
            h = 1e-6 * x.abs().clamp(min=1.0)
            up, dn = torch.where(keep, x + h, x), torch.where(keep, x - h, x)
            d = loss(ins, up, hi) - loss(ins, dn, hi) if which == 0 else loss(ins, lo, up) - loss(ins, lo, dn)
            fd.append(torch.where(keep, d / (2 * h), torch.zeros_like(d)).cpu().numpy())
        err = tr.normwise(grads, fd)[keep_np.any(axis=1)]
        print("%s: reverse mode against central differences of the device op: worst %.2e normwise, %.0f %% of the finite queries kept" % (family, err.max(), 100 * share))
        assert share >= 0.5 and err.max() <= 1e-6, family
        if family != "random":
            continue
        # a (k,) window is every problem's; both None: k = 1, the whole spline; vel0 / vel2 of None are zeros
        z = np.zeros(n)
        flat = [sp[0], sp[1], sp[2], z, z, sp[5], sp[6], sp[7]]
        six = [ins[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")]
        row_lo, row_hi = _t(np.array([0.1, 0.2, 0.3])).requires_grad_(), _t(np.array([0.5, 0.25, 9.0]))
        o = rp.trajectory_integrals(*six, row_lo, row_hi)
        want = _int(flat, np.repeat([[0.1, 0.2, 0.3]], n, axis=0), np.repeat([[0.5, 0.25, 9.0]], n, axis=0))
        assert all(_same_bits(a.detach().cpu().numpy(), b) for a, b in zip(o, want))
        (g_row,) = torch.autograd.grad(torch.nan_to_num(o[1]).sum(), row_lo)
        assert g_row.shape == (3,)
        whole = rp.trajectory_integrals(*six)
        assert whole[0].shape == (n, 1) and all(_same_bits(a.cpu().numpy(), b) for a, b in zip(whole, _int(flat, None, None, k=1)))
        only_hi = rp.trajectory_integrals(*six, None, row_hi)
        assert all(_same_bits(a.cpu().numpy(), b) for a, b in zip(only_hi, _int(flat, None, np.repeat([[0.5, 0.25, 9.0]], n, axis=0))))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. through the solve
def test_the_pipeline_against_central_differences():
    orc = Oracle()
    n, k = 4096, 8
    args = tg._inputs(orc, 0.1, n)
    names = ("pos0", "pos1", "pos2", "vel0", "vel2")
    x = {nm: _t(a).requires_grad_() for nm, a in zip(names, args)}

    def pipeline(v, a, b):
        return rp.min_time_integrals(v["pos0"], v["pos1"], v["pos2"], a, b, vel0=v["vel0"], vel2=v["vel2"], gap_tol=1e-13)

    with torch.no_grad():
        first = pipeline(x, None, None)
    sol = [t.cpu().numpy() for t in first[4:7]]
    live = np.isfinite(np.stack(sol, 1)).all(1) & (sol[1] > 0) & (sol[2] > 0)
    sp = [np.where(live, a, 1.0) for a in tuple(args) + tuple(sol)]
    lo_np, hi_np = xr.windows(sp, k, 23)      # fixed times: the windows do not move with the solution
    lo, hi = _t(lo_np), _t(hi_np)
    out = pipeline(x, lo, hi)
    assert len(out) == 9
    status = out[8]
    keep_rule = ir.kept_for_differences(sp, lo_np, hi_np)
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
    for j, name in enumerate(ir.NAMES):
        finite = conv[:, None] & np.isfinite(out[j].detach().cpu().numpy())
        keep_np = finite & keep_rule
        share = keep_np.sum() / finite[:, [0] + list(range(2, k))].sum()
        keep = _t(keep_np).bool()
        rows = lambda o: torch.where(keep, wt * o, torch.zeros_like(wt)).sum(1)      # noqa: E731
        grads = torch.autograd.grad(rows(out[j]).sum(), [x[nm] for nm in names], retain_graph=True)
        print("%s: %.0f %% of the converged, finite queries kept" % (name, 100 * share))
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
