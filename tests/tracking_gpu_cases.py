"""The cases of tests/test_gpu_tracking.py, each run in a fresh process (`python tests/tracking_gpu_cases.py <case> [family]`), on top of
tests/trajectory_gpu_cases.py's and tests/gap_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is
checked, and why each bound is what it is: DESIGN.md section 20."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gap_gpu_cases as gg  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import gap_ref as gr  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import tracking_ref as kr  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

N, SHAPES, LD, NAMES = gg.N, gg.SHAPES, np.longdouble, gg.NAMES
_t, _same_bits, _head, Out = gg._t, gg._same_bits, gg._head, gg.Out
ALL = (True, True, True)


def _family(name, n=N):
    if name == "dyadic":
        a, b, _, _, delay = kr.dyadic_cases()
        return a, b, lambda k, seed: np.repeat(delay, k, axis=1)
    return gg._family(name, n)


def _queries(name, a, b, delays, k, seed):
    if name == "dyadic":
        _, _, lo, hi, delay = kr.dyadic_cases()
        return np.repeat(lo, k, axis=1), np.repeat(hi, k, axis=1), np.repeat(delay, k, axis=1)
    return gg._queries(name, a, b, delays, k, seed)


def _addr(x):
    return x.data_ptr() if x is not None else 0


def _splines(a, b, zero_vel=False):
    ta, tb = [_t(x) for x in a], [_t(x) for x in b]
    addr_a, addr_b = [t.data_ptr() for t in ta], [t.data_ptr() for t in tb]
    if zero_vel:
        addr_a[3] = addr_a[4] = addr_b[3] = addr_b[4] = 0
    return (ta, tb), addr_a, addr_b


def _shape(a, lo, hi, delay, k):
    return len(a[0]), k if k is not None else next(x for x in (lo, hi, delay) if x is not None).shape[1]


def _track(a, b, lo, hi, delay, k=None, want=ALL, zero_vel=False):
    """The stateless entry: three values, None where not asked for.  lo / hi / delay of None go in as NULL."""
    n, k = _shape(a, lo, hi, delay, k)
    keep, addr_a, addr_b = _splines(a, b, zero_vel)
    q = [_t(x) if x is not None else None for x in (lo, hi, delay)]
    outs = [Out(n, k) if w else None for w in want]
    capi.trajectory_tracking(0, 0, n, k, addr_a, addr_b, *[_addr(x) for x in q], [o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _tvjp(a, b, lo, hi, delay, g, k=None, want_a=(True,) * 8, want_b=(True,) * 8, want_q=ALL):
    """g: three (n, k) arrays or None each, or None (a NULL table).  Returns (A's eight bars, B's eight, [lo_bar, hi_bar, delay_bar])."""
    n, k = _shape(a, lo, hi, delay, k)
    keep, addr_a, addr_b = _splines(a, b)
    q = [_t(x) if x is not None else None for x in (lo, hi, delay)]
    gs = [_t(x) if x is not None else None for x in g] if g is not None else None
    bars_a, bars_b = [Out(n) if w else None for w in want_a], [Out(n) if w else None for w in want_b]
    qb = [Out(n, k) if w else None for w in want_q]
    capi.trajectory_tracking_vjp(0, 0, n, k, addr_a, addr_b, *[_addr(x) for x in q], [_addr(x) for x in gs] if gs is not None else None,
                                 [o.ptr if o else 0 for o in bars_a], [o.ptr if o else 0 for o in bars_b], *[o.ptr if o else 0 for o in qb])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in bars_a], [o.get() if o else None for o in bars_b], [o.get() if o else None for o in qb]


def _tjvp(a, b, lo, hi, delay, a_dot, b_dot, lo_dot, hi_dot, delay_dot, k=None, want=ALL):
    n, k = _shape(a, lo, hi, delay, k)
    keep, addr_a, addr_b = _splines(a, b)
    q = [_t(x) if x is not None else None for x in (lo, hi, delay, lo_dot, hi_dot, delay_dot)]
    da = [_t(x) if x is not None else None for x in a_dot] if a_dot is not None else None
    db = [_t(x) if x is not None else None for x in b_dot] if b_dot is not None else None
    outs = [Out(n, k) if w else None for w in want]
    capi.trajectory_tracking_jvp(0, 0, n, k, addr_a, addr_b, *[_addr(x) for x in q[:3]], [_addr(x) for x in da] if da is not None else None,
                                 [_addr(x) for x in db] if db is not None else None, *[_addr(x) for x in q[3:]], [o.ptr if o else 0 for o in outs])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in outs]


def _flat(v):
    return v[0] + v[1] + v[2] if isinstance(v, tuple) else v


def _all_same(x, y):
    return all((p is None and q is None) or _same_bits(p, q) for p, q in zip(_flat(x), _flat(y)))


def _directions(n, k, seed):
    rng = np.random.default_rng(seed)
    return ([rng.standard_normal(n) for _ in range(8)], [rng.standard_normal(n) for _ in range(8)], rng.standard_normal((n, k)),
            rng.standard_normal((n, k)), rng.standard_normal((n, k)))


# ---------------------------------------------------------------- 1. forward
def test_forward_against_the_definition(family):
    """The CPU table's bounds (tracking_ref.FORWARD_BOUNDS, of the output's scale): NaN mask identical, exact zeros where a == b; the
    follower with no delay: relvel_sq exactly 0, gap_int and gap_sq 25 and 625 times the window to the same bounds."""
    worst = [0.0, 0.0, 0.0]
    shapes = ((4, 1), (4, 7), (4, 8)) if family == "dyadic" else SHAPES
    for n, k in shapes:
        a, b, delays = _family(family, n)
        lo, hi, delay = _queries(family, a, b, delays, k, 300 + k)
        want = kr.tracking_ld(a, b, lo, hi, delay)
        walk = kr._walk(a, b, lo, hi, delay, LD)
        got = _track(a, b, lo, hi, delay)
        sc = kr.value_scales(a, b)
        for j, name in enumerate(kr.NAMES):
            missing = np.isnan(np.asarray(want[j], dtype=np.float64))
            assert np.array_equal(np.isnan(got[j]), missing), (family, n, k, name, "the NaN mask")
            assert np.all(got[j][walk["empty"]] == 0.0) and not np.any(np.signbit(got[j][walk["empty"]])), (family, n, k, name, "a == b")
            err = float(np.where(missing, 0, np.asarray(np.abs(got[j] - want[j]) / sc[j], dtype=np.float64)).max())
            worst[j] = max(worst[j], err)
            if family == "follower0":
                length = np.asarray(walk["b"].astype(LD) - walk["a"].astype(LD))
                exact = (25 * length, 625 * length, 0 * length)[j]
                if j == 2:
                    assert np.all(got[j][~missing] == 0.0), (n, k, "relvel_sq is exactly 0")
                assert float(np.where(missing, 0, np.asarray(np.abs(got[j] - exact) / sc[j], dtype=np.float64)).max()) <= kr.FORWARD_BOUNDS[j], (n, k, name)
    for j, name in enumerate(kr.NAMES):
        print("%s, %s: worst error %.3g of the scale (bound %.3g)" % (family, name, worst[j], kr.FORWARD_BOUNDS[j]))
        assert worst[j] <= kr.FORWARD_BOUNDS[j], (family, name, worst[j])
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. NULLs and the NaN rule
def test_nulls_and_the_nan_rule():
    for n, k in SHAPES:
        a, b, delays = _family("random", n)
        lo, hi, delay = _queries("random", a, b, delays, k, 400 + k)
        full = _track(a, b, lo, hi, delay)
        inf, zero = np.full((n, k), np.inf), np.zeros((n, k))
        # NULL lo / hi / delay / all three against explicit -inf, +inf and zeros
        assert _all_same(_track(a, b, None, hi, delay), _track(a, b, -inf, hi, delay))
        assert _all_same(_track(a, b, lo, None, delay), _track(a, b, lo, inf, delay))
        assert _all_same(_track(a, b, lo, hi, None), _track(a, b, lo, hi, zero))
        assert _all_same(_track(a, b, None, None, None, k=k), _track(a, b, -inf, inf, zero))
        # each output alone, and each alone left out (the sentinels behind every buffer are checked by Out.get)
        for j in range(3):
            alone = _track(a, b, lo, hi, delay, want=tuple(i == j for i in range(3)))
            without = _track(a, b, lo, hi, delay, want=tuple(i != j for i in range(3)))
            assert _same_bits(alone[j], full[j]) and all(x is None for i, x in enumerate(alone) if i != j), (n, k, j)
            assert without[j] is None and all(_same_bits(without[i], full[i]) for i in range(3) if i != j), (n, k, j)
        # NULL end velocities against zeros
        za, zb = [x.copy() for x in a], [x.copy() for x in b]
        for s in (za, zb):
            s[3][:] = 0.0
            s[4][:] = 0.0
        assert _all_same(_track(za, zb, lo, hi, delay, zero_vel=True), _track(za, zb, lo, hi, delay))
        # the NaN rule: exactly that problem or query goes NaN, and no other bit changes
        for side in range(2):
            for row, (f, bad) in enumerate(((6, 0.0), (7, -1.0), (6, np.inf), (7, np.nan))):
                if row >= n:
                    continue
                pa, pb = [x.copy() for x in a], [x.copy() for x in b]
                (pb if side else pa)[f][row] = bad
                got = _track(pa, pb, lo, hi, delay)
                for j in range(3):
                    assert np.all(np.isnan(got[j][row])), (n, k, side, f, bad)
                    assert _same_bits(np.delete(got[j], row, axis=0), np.delete(full[j], row, axis=0)), (n, k, side, f, bad)
        rng = np.random.default_rng(7 + k)
        for which, bad in ((0, np.nan), (1, np.nan), (2, np.nan), (2, np.inf), (2, -np.inf)):
            q = [lo.copy(), hi.copy(), delay.copy()]
            hit = rng.random((n, k)) < 0.1
            q[which][hit] = bad
            got = _track(a, b, *q)
            for j in range(3):
                assert np.all(np.isnan(got[j][hit])), (n, k, which, bad)
                assert _same_bits(got[j][~hit], full[j][~hit]), (n, k, which, bad)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 3. bits
def test_bits_depend_on_the_problem_and_its_query_only():
    """The call made twice, the problems permuted, rows as batches of their own (1, 129, the last 44), and the k = 7 columns inside a k = 8
    launch: the same bits, for the forward, the JVP and the VJP's per-problem gradients."""
    n = N
    a, b, delays = _family("random", n)
    for k in (7, 8):
        lo, hi, delay = _queries("random", a, b, delays, k, 500 + k)
        g = gg.tg._gradients(n, k, 51)
        ad, bd, lod, hid, dld = _directions(n, k, 52)

        def run(rows):
            sa, sb = [x[rows] for x in a], [x[rows] for x in b]
            q = [x[rows] for x in (lo, hi, delay)]
            fwd = _track(sa, sb, *q)
            jv = _tjvp(sa, sb, *q, [x[rows] for x in ad], [x[rows] for x in bd], lod[rows], hid[rows], dld[rows])
            va, vb, vq = _tvjp(sa, sb, *q, [x[rows] for x in g])
            return fwd + jv + va + vb + vq

        full = run(slice(None))
        assert _all_same(full, run(slice(None))), (k, "the same call twice")
        perm = np.random.default_rng(53).permutation(n)
        assert all(_same_bits(x[perm], y) for x, y in zip(full, run(perm))), (k, "permuted")
        for rows in (slice(5, 6), slice(100, 229), slice(n - 44, n)):
            assert all(_same_bits(x[rows], y) for x, y in zip(full, run(rows))), (k, rows)
    # the k = 7 queries as the first seven columns of a k = 8 launch: the pointwise outputs' bits (the gradients sum over other queries)
    lo7, hi7, dl7 = _queries("random", a, b, delays, 7, 507)
    pad = lambda x, v: np.ascontiguousarray(np.concatenate([x, np.full((n, 1), v)], axis=1))      # noqa: E731
    lo8, hi8, dl8 = pad(lo7, -np.inf), pad(hi7, np.inf), pad(dl7, 0.0)
    ad, bd, lod, hid, dld = _directions(n, 7, 54)
    seven = _track(a, b, lo7, hi7, dl7) + _tjvp(a, b, lo7, hi7, dl7, ad, bd, lod, hid, dld)
    eight = _track(a, b, lo8, hi8, dl8) + _tjvp(a, b, lo8, hi8, dl8, ad, bd, pad(lod, 0.0), pad(hid, 0.0), pad(dld, 0.0))
    assert all(_same_bits(x, y[:, :7]) for x, y in zip(seven, eight))
    g7 = gg.tg._gradients(n, 7, 55)
    q7 = _tvjp(a, b, lo7, hi7, dl7, g7)[2]
    q8 = _tvjp(a, b, lo8, hi8, dl8, [pad(x, 0.0) for x in g7])[2]
    assert all(_same_bits(x, y[:, :7]) for x, y in zip(q7, q8))
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 4. the derivative entries
def test_vjp_and_jvp_against_longdouble(family):
    """Normwise per problem against vjp_ld / jvp_ld; the bound is section 15's rule: ten times the worst error of the float64 restatement
    of the same rule on the same inputs."""
    for n, k in SHAPES:
        a, b, delays = _family(family, n)
        lo, hi, delay = _queries(family, a, b, delays, k, 600 + k)
        g = gg.tg._gradients(n, k, 61)
        ad, bd, lod, hid, dld = _directions(n, k, 62)
        want, f64 = kr.vjp_ld(a, b, lo, hi, delay, g), kr.vjp_f64(a, b, lo, hi, delay, g)
        got = _tvjp(a, b, lo, hi, delay, g)
        stack = lambda v: list(v[0]) + list(v[1]) + list(v[2:] if len(v) == 5 else v[2])      # noqa: E731
        ref_err = np.nanmax(tr.normwise(stack(f64), stack(want)))
        dev_err = tr.normwise(stack(got), stack(want))
        assert np.all(np.isfinite(np.concatenate([x.ravel() for x in stack(got)]))), (family, n, k, "a gradient is not finite")
        print("%s %d x %d reverse: device %.3g, the float64 restatement %.3g" % (family, n, k, np.nanmax(dev_err), ref_err))
        assert np.nanmax(dev_err) <= 10 * ref_err, (family, n, k, np.nanmax(dev_err), ref_err)
        want, f64 = (fn(a, b, lo, hi, delay, ad, bd, lod, hid, dld) for fn in (kr.jvp_ld, kr.jvp_f64))
        got = _tjvp(a, b, lo, hi, delay, ad, bd, lod, hid, dld)
        missing = np.isnan(np.asarray(want[0], dtype=np.float64))
        assert all(np.array_equal(np.isnan(x), missing) for x in got), (family, n, k, "the NaN mask of the tangents")
        z = lambda v: [np.where(missing, 0, x) for x in v]      # noqa: E731
        ref_err = np.nanmax(tr.normwise(z(f64), z(want)))
        dev_err = np.nanmax(tr.normwise(z(got), z(want)))
        print("%s %d x %d forward: device %.3g, the float64 restatement %.3g" % (family, n, k, dev_err, ref_err))
        assert dev_err <= 10 * ref_err, (family, n, k, dev_err, ref_err)
        # NULL gradients and tangents against explicit zeros; each VJP output alone
        zero, zn = np.zeros((n, k)), np.zeros(n)
        assert _all_same(_tvjp(a, b, lo, hi, delay, [g[0], None, g[2]]), _tvjp(a, b, lo, hi, delay, [g[0], zero, g[2]]))
        assert _all_same(_tvjp(a, b, lo, hi, delay, None), _tvjp(a, b, lo, hi, delay, [zero, zero, zero]))
        assert _all_same(_tjvp(a, b, lo, hi, delay, None, [None] * 7 + [bd[7]], None, hid, None),
                         _tjvp(a, b, lo, hi, delay, [zn] * 8, [zn] * 7 + [bd[7]], zero, hid, zero))
        if k == 8:
            full = _tvjp(a, b, lo, hi, delay, g)
            none8 = (False,) * 8
            for f in range(19):
                wa = tuple(i == f for i in range(8))
                wb = tuple(i == f - 8 for i in range(8))
                wq = tuple(i == f - 16 for i in range(3))
                one = _tvjp(a, b, lo, hi, delay, g, want_a=wa if f < 8 else none8, want_b=wb if 8 <= f < 16 else none8, want_q=wq)
                assert _same_bits(_flat(one)[f], _flat(full)[f]) and sum(x is not None for x in _flat(one)) == 1, f
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. autograd
def _leaves(a, b, lo, hi, delay):
    ins_a = {nm: _t(x).requires_grad_() for nm, x in zip(NAMES, a)}
    ins_b = {nm: _t(x).requires_grad_() for nm, x in zip(NAMES, b)}
    return ins_a, ins_b, [_t(x).requires_grad_() for x in (lo, hi, delay)]


def _run(ins_a, ins_b, lo, hi, delay):
    six = lambda d: [d[nm] for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1", "vel0", "vel2")]      # noqa: E731
    return rp.trajectory_tracking(six(ins_a), six(ins_b), lo, hi, delay)


def test_autograd_reverse_forward_and_duality():
    n, k = N, 8
    a, b, delays = _family("random", n)
    lo_np, hi_np, dl_np = _queries("random", a, b, delays, k, 700)
    ins_a, ins_b, (lo, hi, delay) = _leaves(a, b, lo_np, hi_np, dl_np)
    leaves = [ins_a[nm] for nm in NAMES] + [ins_b[nm] for nm in NAMES] + [lo, hi, delay]
    outs = _run(ins_a, ins_b, lo, hi, delay)
    want = _track(a, b, lo_np, hi_np, dl_np)
    assert all(_same_bits(x.detach().cpu().numpy(), y) for x, y in zip(outs, want))
    g = gg.tg._gradients(n, k, 71)
    missing = np.isnan(want[0])
    # a NaN output contributes exactly 0 whatever its upstream gradient, and all gradients are finite
    wild = [np.where(missing, 1e300, x) for x in g]
    grads = torch.autograd.grad(outs, leaves, [_t(x) for x in g], retain_graph=True)
    grads_wild = torch.autograd.grad(outs, leaves, [_t(x) for x in wild], retain_graph=True)
    dev = _tvjp(a, b, lo_np, hi_np, dl_np, g)
    for x, y, z in zip(grads, grads_wild, _flat(dev)):
        assert torch.isfinite(x).all() and _same_bits(x.cpu().numpy(), y.cpu().numpy()) and _same_bits(x.cpu().numpy(), z)
    assert missing.any() and np.all(grads[16].cpu().numpy()[missing] == 0) and np.all(grads[18].cpu().numpy()[missing] == 0)
    # forward mode: forward_ad and torch.func.jvp give the entry's bits
    ad, bd, lod, hid, dld = _directions(n, k, 72)
    dots = [_t(x) for x in ad] + [_t(x) for x in bd] + [_t(lod), _t(hid), _t(dld)]
    with fwAD.dual_level():
        duals = [fwAD.make_dual(x.detach(), d) for x, d in zip(leaves, dots)]
        da, db = dict(zip(NAMES, duals[:8])), dict(zip(NAMES, duals[8:16]))
        tang = [fwAD.unpack_dual(o).tangent for o in _run(da, db, *duals[16:])]
    dev_j = _tjvp(a, b, lo_np, hi_np, dl_np, ad, bd, lod, hid, dld)
    assert all(_same_bits(x.cpu().numpy(), y) for x, y in zip(tang, dev_j))
    fn = lambda *xs: _run(dict(zip(NAMES, xs[:8])), dict(zip(NAMES, xs[8:16])), *xs[16:])      # noqa: E731
    _, func_tang = torch.func.jvp(fn, tuple(x.detach() for x in leaves), tuple(dots))
    assert all(_same_bits(x.cpu().numpy(), y.cpu().numpy()) for x, y in zip(func_tang, tang))
    # duality between the modes, to 1e-12 of the sum of |terms|
    lhs_terms = [np.where(missing, 0, gi * ti.cpu().numpy()) for gi, ti in zip(g, tang)]
    rhs_terms = [gr_.cpu().numpy() * d.cpu().numpy() for gr_, d in zip(grads, dots)]
    lhs, rhs = sum(x.sum() for x in lhs_terms), sum(x.sum() for x in rhs_terms)
    size = sum(np.abs(x).sum() for x in lhs_terms) + sum(np.abs(x).sum() for x in rhs_terms)
    print("duality: |<g, J d> - <J^T g, d>| = %.3g of the sum of |terms|" % (abs(lhs - rhs) / size))
    assert abs(lhs - rhs) <= 1e-12 * size
    # only the gradients asked for; a (k,) row of queries; all None: k = 1; a double backward raises
    (only,) = torch.autograd.grad(outs[1].nan_to_num().sum(), [ins_b["duration1"]], retain_graph=True)
    ones = [None, np.where(missing, 0.0, 1.0), None]
    assert _same_bits(only.cpu().numpy(), _tvjp(a, b, lo_np, hi_np, dl_np, ones)[1][7])
    row = _t(np.array([0.01, -0.02, 0.0])).requires_grad_()
    six_a = [ins_a[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")]
    six_b = [ins_b[nm].detach() for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1")]
    flat_a, flat_b = [x.copy() for x in a], [x.copy() for x in b]
    for s in (flat_a, flat_b):
        s[3][:] = 0.0
        s[4][:] = 0.0
    o = rp.trajectory_tracking(six_a, six_b, None, None, row)
    assert all(_same_bits(x.detach().cpu().numpy(), y) for x, y in zip(o, _track(flat_a, flat_b, None, None, np.repeat(row.detach().cpu().numpy()[None, :], n, axis=0))))
    (g_row,) = torch.autograd.grad(o[0].nan_to_num().sum(), row)
    assert g_row.shape == (3,)
    whole = rp.trajectory_tracking(six_a, six_b)
    assert whole[0].shape == (n, 1) and all(_same_bits(x.cpu().numpy(), y) for x, y in zip(whole, _track(flat_a, flat_b, None, None, None, k=1)))
    (first,) = torch.autograd.grad((outs[1].nan_to_num() ** 2).sum(), [ins_a["pos1"]], create_graph=True)
    try:
        first.sum().backward()
    except RuntimeError as e:
        assert "once_differentiable" in str(e), e
    else:
        raise AssertionError("a double backward did not raise")
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 6. through the solves
def test_the_pipeline_against_central_differences():
    """min_time_tracking on 300 golden problems against themselves 25 lower, delays U(0.02, 0.3) T, against central differences of the whole
    device pipeline in pos1 of each vehicle, h = 1e-4: section 15's pipeline bound, median < 1e-5 and 95 % < 1e-3 on converged finite
    queries, in more than half of the problems."""
    n, k = N, 8
    pos = gg._golden_positions(n)
    xa = [_t(pos[:, c]).requires_grad_() for c in range(3)]
    xb = [_t(pos[:, c] - 25.0).requires_grad_() for c in range(3)]

    def pipeline(pa, pb, lo, hi, delay):
        return rp.min_time_tracking(pa, pb, lo, hi, delay, gap_tol=1e-13)

    with torch.no_grad():
        first = pipeline(xa, xb, None, None, None)
    assert len(first) == 5 and len(first[3]) == 5 and len(first[4]) == 5
    sols = [[t.cpu().numpy() for t in s[:3]] for s in first[3:]]
    conv = np.ones(n, dtype=bool)
    for s, status in zip(sols, (first[3][4], first[4][4])):
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
    wt = _t(np.random.default_rng(25).uniform(0.5, 1.5, (n, k)))
    h = 1e-4
    moved = {}
    with torch.no_grad():
        for which in range(2):
            up, dn = [list(xa), list(xb)], [list(xa), list(xb)]
            up[which][1], dn[which][1] = up[which][1] + h, dn[which][1] - h
            moved[which] = (pipeline(up[0], up[1], lo, hi, delay)[:3], pipeline(dn[0], dn[1], lo, hi, delay)[:3])
    for j, name in enumerate(kr.NAMES):
        keep_np = conv[:, None] & np.isfinite(out[j].detach().cpu().numpy())
        for which in range(2):
            keep_np &= np.isfinite(moved[which][0][j].cpu().numpy()) & np.isfinite(moved[which][1][j].cpu().numpy())
        keep = _t(keep_np).bool()
        rows = lambda o: torch.where(keep, wt * o, torch.zeros_like(wt)).sum(1)      # noqa: E731
        grads = torch.autograd.grad(rows(out[j]).sum(), [xa[1], xb[1]], retain_graph=True)
        some = _t(keep_np.any(axis=1)).bool()
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
