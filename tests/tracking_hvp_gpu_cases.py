"""The cases of tests/test_gpu_tracking_hvp.py, each run in a fresh process (`python tests/tracking_hvp_gpu_cases.py <case> [family]`), on
top of tests/tracking_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is checked, and why each bound
is what it is: DESIGN.md section 23."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import tracking_gpu_cases as tc  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import gap_ref as gr  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import tracking_hvp_ref as hr  # noqa: E402
import tracking_ref as kr  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

gg = tc.gg
N, NAMES, LD = 300, tc.NAMES, np.longdouble
NS = (1, 127, 128, 129, 300)            # a block stages 128 problems per trip: one short of a trip, a full one, one over, three trips
KS = (1, 2, 7, 8, 65)                   # single elements and 16-byte pairs, one lane and many, more units than the 64 lanes
GRID_N = 300001                         # 2,344 trips of 128 for the grid's 2,048 blocks
CPU_BOUND = 1e-12                       # tests/test_tracking_hvp_cpu.py's bound on the float64 restatement, normwise per problem
_t, _same_bits, Out, _addr = tc._t, tc._same_bits, tc.Out, tc._addr
ALL8, ALL3 = (True,) * 8, (True,) * 3


def _thvp(a, b, lo, hi, delay, g, a_dot, b_dot, lo_dot, hi_dot, dl_dot, k=None, want_a=ALL8, want_b=ALL8, want_q=ALL3):
    """g: three (n, k) arrays or None each (NULL), or None (a NULL table); a_dot, b_dot: eight arrays of n or None each, or None (a NULL
    table); lo_dot, hi_dot, dl_dot (n, k) or None.  Returns the nineteen results in tracking_hvp_ref.flat's order, None where not asked
    for."""
    n, k = tc._shape(a, lo, hi, delay, k)
    keep, addr_a, addr_b = tc._splines(a, b)
    q = [_t(x) if x is not None else None for x in (lo, hi, delay, lo_dot, hi_dot, dl_dot)]
    table = lambda v: [_t(x) if x is not None else None for x in v] if v is not None else None      # noqa: E731
    gs, da, db = table(g), table(a_dot), table(b_dot)
    ptrs = lambda v: [_addr(x) for x in v] if v is not None else None      # noqa: E731
    bars_a, bars_b = [Out(n) if w else None for w in want_a], [Out(n) if w else None for w in want_b]
    qb = [Out(n, k) if w else None for w in want_q]
    capi.trajectory_tracking_hvp(0, 0, n, k, addr_a, addr_b, *[_addr(x) for x in q[:3]], ptrs(gs), ptrs(da), ptrs(db), *[_addr(x) for x in q[3:]],
                                 [o.ptr if o else 0 for o in bars_a], [o.ptr if o else 0 for o in bars_b], *[o.ptr if o else 0 for o in qb])
    torch.cuda.synchronize()
    return [o.get() if o else None for o in bars_a + bars_b + qb]


def _all_same(x, y):
    return all((p is None and q is None) or (p is not None and q is not None and _same_bits(p, q)) for p, q in zip(x, y))


def _normwise(a, b):
    """The worst of trajectory_ref.normwise over the problems -- where a problem's reference is exactly 0, the norm of the difference
    itself -- and never a NaN."""
    a = np.concatenate([np.asarray(x, dtype=LD).reshape(len(x), -1) for x in a], axis=1)
    b = np.concatenate([np.asarray(x, dtype=LD).reshape(len(x), -1) for x in b], axis=1)
    miss, size = np.linalg.norm((a - b).astype(np.float64), axis=1), np.linalg.norm(b.astype(np.float64), axis=1)
    worst = float(np.max(miss / np.where(size > 0, size, 1.0)))
    assert np.isfinite(worst), "a NaN or infinite result"
    return worst


def _rows(x, rows):
    return [None if v is None else v[rows] for v in x]


def _inputs(family, a, b, delays, k, seed):
    """The family's queries, gradients on all three outputs and a direction in all nineteen inputs."""
    lo, hi, delay = tc._queries(family, a, b, delays, k, seed)
    return (lo, hi, delay), hr.gradients(lo.shape, seed + 3), hr.directions(a, b, lo, hi, delay, seed + 4)


def _call(a, b, q, g, d, rows=slice(None), **kw):
    return _thvp(_rows(a, rows), _rows(b, rows), *_rows(q, rows), _rows(g, rows), _rows(d[0], rows), _rows(d[1], rows), *_rows(d[2:], rows), **kw)


# ---------------------------------------------------------------- 1. the entry against longdouble
def test_entry_against_longdouble_and_nulls(family):
    """Normwise per problem against the longdouble definition: the float64 restatement of the kernel's arithmetic and order first, on the
    same inputs on the CPU; the device is held to 10 x the restatement's worst (DESIGN.md section 15's rule).  The reference is formed once
    per k for the 300 problems, and every smaller n runs its first rows."""
    a, b, delays = tc._family(family, N)
    worst = [0.0, 0.0]      # [restatement, device]
    for k in KS:
        q, g, d = _inputs(family, a, b, delays, k, 2300 + k)
        want = hr.flat(hr.hvp_ld(a, b, *q, g, *d))
        worst[0] = max(worst[0], _normwise(hr.flat(hr.hvp_f64(a, b, *q, g, *d)), want))
        for n in NS:
            worst[1] = max(worst[1], _normwise(_call(a, b, q, g, d, slice(0, n)), _rows(want, slice(0, n))))
        if k not in (7, 8):
            continue
        # every NULL input against explicit zeros: the same bits
        n = 129
        rows = slice(0, n)
        sa, sb, (lo, hi, delay), g, d = _rows(a, rows), _rows(b, rows), _rows(q, rows), _rows(g, rows), [_rows(d[0], rows), _rows(d[1], rows)] + _rows(d[2:], rows)
        full = _thvp(sa, sb, lo, hi, delay, g, *d)
        z, zn = np.zeros((n, k)), np.zeros(n)
        for f in range(3):
            x = _thvp(sa, sb, lo, hi, delay, [None if j == f else v for j, v in enumerate(g)], *d)
            y = _thvp(sa, sb, lo, hi, delay, [z if j == f else v for j, v in enumerate(g)], *d)
            assert _all_same(x, y), (family, k, "g", f)
        assert _all_same(_thvp(sa, sb, lo, hi, delay, None, *d), _thvp(sa, sb, lo, hi, delay, [z] * 3, *d)), (family, k)
        for side in range(2):
            for null in ((True,) * 8, (True, False) * 4, (False, True) * 4):
                dn, dz = list(d), list(d)
                dn[side] = [None if m else v for v, m in zip(d[side], null)]
                dz[side] = [zn if m else v for v, m in zip(d[side], null)]
                assert _all_same(_thvp(sa, sb, lo, hi, delay, g, *dn), _thvp(sa, sb, lo, hi, delay, g, *dz)), (family, k, side, null)
            dn, dz = list(d), list(d)
            dn[side], dz[side] = None, [zn] * 8
            assert _all_same(_thvp(sa, sb, lo, hi, delay, g, *dn), _thvp(sa, sb, lo, hi, delay, g, *dz)), (family, k, side, "the table")
        for at in (2, 3, 4):
            dn, dz = list(d), list(d)
            dn[at], dz[at] = None, z
            assert _all_same(_thvp(sa, sb, lo, hi, delay, g, *dn), _thvp(sa, sb, lo, hi, delay, g, *dz)), (family, k, at)
        # every output alone and alone left out: only what is asked for is written (Out.get checks the sentinels), with the full call's bits
        for f in range(19):
            for alone in (True, False):
                wanted = [(j == f) == alone for j in range(19)]
                some = _thvp(sa, sb, lo, hi, delay, g, *d, want_a=wanted[:8], want_b=wanted[8:16], want_q=wanted[16:])
                for j, x in enumerate(some):
                    assert (x is None) == (not wanted[j]) and (x is None or _same_bits(x, full[j])), (family, k, f, alone, j)
    print("%s: hvp against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, worst[0], worst[1], 10 * worst[0]))
    assert worst[1] <= 10 * worst[0], family


def test_the_nan_rule():
    """A duration of 0, -1, inf, NaN in either spline poisons its problem's sixteen results and no other problem, and its per-query results
    are 0 or NaN where rp_trajectory_tracking_vjp's are; a query whose outputs are NaN (a NaN window end, a NaN or infinite delay) counts
    with gradients of zero and gets three zeros; a NaN lo_dot on a clamped end is not read, on a taken end it makes its own lo_bar_dot NaN;
    every other problem keeps its clean bits."""
    n = 129
    a, b, delays = tc._family("random", n)
    for k in (7, 8):
        (lo, hi, delay), g, d = _inputs("random", a, b, delays, k, 2400 + k)
        clean = _thvp(a, b, lo, hi, delay, g, *d)
        assert all(np.isfinite(x).all() for x in clean)
        for side in range(2):
            pa, pb = [x.copy() for x in a], [x.copy() for x in b]
            rows = (3, 64, 100, 128)
            for row, (f, bad) in zip(rows, ((6, 0.0), (7, -1.0), (6, np.inf), (7, np.nan))):
                (pb if side else pa)[f][row] = bad
            got = _thvp(pa, pb, lo, hi, delay, g, *d)
            first = tc._tvjp(pa, pb, lo, hi, delay, g)
            rest = np.delete(np.arange(n), rows)
            for j, x in enumerate(got):
                if j < 16:
                    assert np.isnan(x[list(rows)]).all(), (k, side, j)
                else:
                    assert np.array_equal(np.isnan(x[list(rows)]), np.isnan(first[2][j - 16][list(rows)])), (k, side, j, "the VJP's mask")
                    assert np.all((x[list(rows)] == 0) | np.isnan(x[list(rows)])), (k, side, j)
                assert _same_bits(x[rest], clean[j][rest]), (k, side, j)
        rng = np.random.default_rng(7 + k)
        for which, bad in ((0, np.nan), (1, np.nan), (2, np.nan), (2, np.inf), (2, -np.inf)):
            q = [lo.copy(), hi.copy(), delay.copy()]
            hit = rng.random((n, k)) < 0.1
            q[which][hit] = bad
            got = _thvp(a, b, *q, g, *d)
            untouched = ~hit.any(axis=1)
            assert untouched.any() and hit.any()
            for j, x in enumerate(got):
                assert np.isfinite(x).all(), (k, which, bad, j)
                if j >= 16:
                    assert np.all(x[hit] == 0) and _same_bits(x[~hit], clean[j][~hit]), (k, which, bad, j)
                else:
                    assert _same_bits(x[untouched], clean[j][untouched]), (k, which, bad, j)
        # the window's start clamped in column 0: its tangent is not read; taken in column 1 of problem 5: its own lo_bar_dot is NaN
        lo2, ld = lo.copy(), d[2].copy()
        lo2[:, 0] = -np.inf
        base = _thvp(a, b, lo2, hi, delay, g, d[0], d[1], ld, d[3], d[4])
        ld[:, 0] = np.nan
        assert _all_same(base, _thvp(a, b, lo2, hi, delay, g, d[0], d[1], ld, d[3], d[4])), k
        walk = kr._walk(a, b, lo2, hi, delay, np.float64)
        row, col = np.argwhere(walk["ok"] & ~walk["empty"] & (walk["cls_a"] == kr.A_LO))[0]
        ld[:, 0] = 0.0
        ld[row, col] = np.nan
        got = _thvp(a, b, lo2, hi, delay, g, d[0], d[1], ld, d[3], d[4])
        assert np.isnan(got[16][row, col]), k
        rest = np.delete(np.arange(n), row)
        assert all(_same_bits(x[rest], y[rest]) for x, y in zip(got, base)), k
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 2. reproducibility
def test_bits_depend_on_the_problem_and_k_only():
    roll = lambda x: np.concatenate([x[1:], x[:1]])      # noqa: E731
    for family in ("random", "follower"):
        a, b, delays = tc._family(family, N)
        for k in KS:
            q, g, d = _inputs(family, a, b, delays, k, 2500 + k)
            big = _call(a, b, q, g, d)
            assert _all_same(big, _call(a, b, q, g, d)), (family, k, "differs from run to run")
            for n in NS[:-1]:
                assert _all_same(_call(a, b, q, g, d, slice(0, n)), _rows(big, slice(0, n))), (family, n, k)
            moved = _thvp([roll(x) for x in a], [roll(x) for x in b], *[roll(x) for x in q], [roll(x) for x in g], [roll(x) for x in d[0]],
                          [roll(x) for x in d[1]], *[roll(x) for x in d[2:]])
            for x, y in zip(moved, big):      # problem 0 moved to the end
                assert _same_bits(x[-1], y[0]) and _same_bits(x[:-1], y[1:]), (family, k)
        # the k = 7 queries as the first seven columns of a k = 8 launch: the per-query results' bits (the per-problem ones sum over the eighth)
        q, g, d = _inputs(family, a, b, delays, 7, 2507)
        pad = lambda x, v: np.ascontiguousarray(np.concatenate([x, np.full((N, 1), v)], axis=1))      # noqa: E731
        seven = _call(a, b, q, g, d)[16:]
        eight = _thvp(a, b, pad(q[0], -np.inf), pad(q[1], np.inf), pad(q[2], 0.0), [pad(x, 0.0) for x in g], d[0], d[1], *[pad(x, 0.0) for x in d[2:]])[16:]
        assert all(_same_bits(x, y[:, :7]) for x, y in zip(seven, eight)), family
    # more trips than the grid's cap: 300,001 pairs of one query each
    n = GRID_N
    a, b = gr.random_pair(n)
    delay = gr.delays(a, b, 1, 77)
    lo, hi = gr.windows(a, b, delay, 78)
    g, d = hr.gradients(lo.shape, 79), hr.directions(a, b, lo, hi, delay, 80)
    got = _thvp(a, b, lo, hi, delay, g, *d)
    f64 = hr.flat(hr.hvp_f64(a, b, lo, hi, delay, g, *d))
    err = _normwise(got, f64)
    print("%d pairs x 1 query against the float64 restatement, normwise: worst %.2e; asserted %.0e" % (n, err, CPU_BOUND))
    assert err <= CPU_BOUND


# ---------------------------------------------------------------- 3. identities on the device
def _miss_of_parts(parts, whole, n):
    """|sum of parts - whole| and the sum of |terms| per problem, over all nineteen results."""
    miss_all, size_all = LD(0), LD(0)
    for j, c in enumerate(whole):
        p = [x[j].astype(LD) for x in parts]
        size_all = size_all + (sum(np.abs(x) for x in p) + np.abs(c)).reshape(n, -1).sum(axis=1)
        miss_all = miss_all + np.abs(sum(p) - c.astype(LD)).reshape(n, -1).sum(axis=1)
    out = np.asarray(miss_all / np.where(size_all > 0, size_all, LD(1)), dtype=np.float64)
    assert np.isfinite(out).all()
    return float(out.max())


def test_symmetry_and_linearity_on_the_device():
    """u^T H[g] v = v^T H[g] u; each g alone, summed, is all three; the direction in A (and the queries) alone plus that in B alone is
    both: each within 1e-12 of the sum of |terms| per problem (section 19's bounds for the same identities)."""
    worst_sym = worst_lin = worst_side = 0.0
    for family in ("random", "solved", "follower"):
        a, b, delays = tc._family(family, N)
        for k in KS:
            lo, hi, delay = tc._queries(family, a, b, delays, k, 2700 + k)
            g = hr.gradients(lo.shape, 2701 + k)
            u, v = hr.directions(a, b, lo, hi, delay, 2702 + k), hr.directions(a, b, lo, hi, delay, 2703 + k)
            Hv, Hu = _thvp(a, b, lo, hi, delay, g, *v), _thvp(a, b, lo, hi, delay, g, *u)
            split = lambda r: (r[:8], r[8:16], r[16], r[17], r[18])      # noqa: E731
            left, size_l = hr.bilinear(split(Hv), u)
            right, size_r = hr.bilinear(split(Hu), v)
            sym = np.asarray(np.abs(left - right) / (size_l + size_r), dtype=np.float64)
            assert np.isfinite(sym).all(), (family, k)
            worst_sym = max(worst_sym, float(sym.max()))
            alone = [_thvp(a, b, lo, hi, delay, [x if j == f else None for j, x in enumerate(g)], *v) for f in range(3)]
            worst_lin = max(worst_lin, _miss_of_parts(alone, Hv, N))
            sides = [_thvp(a, b, lo, hi, delay, g, v[0], None, v[2], v[3], v[4]), _thvp(a, b, lo, hi, delay, g, None, v[1], None, None, None)]
            worst_side = max(worst_side, _miss_of_parts(sides, Hv, N))
    print("symmetry %.2e, linearity in g %.2e, side A alone + side B alone %.2e of the sum of |terms| per problem; asserted 1e-12 each"
          % (worst_sym, worst_lin, worst_side))
    assert worst_sym <= 1e-12 and worst_lin <= 1e-12 and worst_side <= 1e-12


# ---------------------------------------------------------------- 4. autograd
def _run(ins_a, ins_b, lo, hi, delay, order):
    six = lambda d: [d[nm] for nm in ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1", "vel0", "vel2")]      # noqa: E731
    return rp.trajectory_tracking(six(ins_a), six(ins_b), lo, hi, delay, order=order)


def test_autograd_order_2():
    n, k = N, 7
    for family in ("random", "follower"):
        a, b, delays = tc._family(family, n)
        lo_np, hi_np, dl_np = tc._queries(family, a, b, delays, k, 2800)
        g_np = hr.gradients(lo_np.shape, 2801)
        d_np = hr.directions(a, b, lo_np, hi_np, dl_np, 2802)
        ins_a, ins_b, (lo, hi, delay) = tc._leaves(a, b, lo_np, hi_np, dl_np)
        leaves = [ins_a[nm] for nm in NAMES] + [ins_b[nm] for nm in NAMES] + [lo, hi, delay]
        g = [_t(x).requires_grad_() for x in g_np]
        u = [_t(x) for x in d_np[0]] + [_t(x) for x in d_np[1]] + [_t(x) for x in d_np[2:]]
        numpy = lambda xs: [x.detach().cpu().numpy() for x in xs]      # noqa: E731

        # forward, backward (create_graph False and True), one output used, and forward mode: order=1's bits
        first = {}
        for order in (1, 2):
            outs = _run(ins_a, ins_b, lo, hi, delay, order)
            first[order, "out"] = numpy(outs)
            for create_graph in (False, True):
                if order == 1 and create_graph:
                    continue
                grads = torch.autograd.grad(outs, leaves, grad_outputs=[x.detach() for x in g], create_graph=create_graph, retain_graph=True)
                first[order, create_graph] = numpy(grads)
            only = torch.autograd.grad((g[1].detach() * torch.nan_to_num(_run(ins_a, ins_b, lo, hi, delay, order)[1])).sum(), leaves)
            first[order, "only"] = numpy(only)
            with fwAD.dual_level():
                duals = [fwAD.make_dual(x.detach(), dx) for x, dx in zip(leaves, u)]
                outs = _run(dict(zip(NAMES, duals[:8])), dict(zip(NAMES, duals[8:16])), *duals[16:], order)
                first[order, "jvp"] = [fwAD.unpack_dual(x).tangent.cpu().numpy() for x in outs]
        for key in ("out", False, "only", "jvp"):
            assert _all_same(first[1, key], first[2, key]), (family, key)
        assert _all_same(first[1, False], first[2, True]), family
        assert _all_same(first[2, True], tc._flat(tc._tvjp(a, b, lo_np, hi_np, dl_np, g_np))), family

        # the double backward of a scalar loss: in the spline inputs and the queries the hvp entry, in the first backward's grad_outputs the
        # jvp entry (NaN where the output is)
        grads = torch.autograd.grad(_run(ins_a, ins_b, lo, hi, delay, 2), leaves, grad_outputs=g, create_graph=True)
        s = sum((gr_ * x).sum() for gr_, x in zip(grads, u))
        second = torch.autograd.grad(s, leaves + g, retain_graph=True)
        want = _thvp(a, b, lo_np, hi_np, dl_np, g_np, *d_np) + tc._tjvp(a, b, lo_np, hi_np, dl_np, *d_np)
        assert _all_same(numpy(second), want), family
        # a loss on gap_sq alone, differentiated the second time along A's pos1 and the delay alone: NULL gradients and NULL directions
        grads = torch.autograd.grad(_run(ins_a, ins_b, lo, hi, delay, 2)[1], [ins_a["pos1"], delay], grad_outputs=g[1].detach(), create_graph=True)
        s = (grads[0] * u[1]).sum() + (grads[1] * u[18]).sum()
        second = torch.autograd.grad(s, leaves)
        want = _thvp(a, b, lo_np, hi_np, dl_np, [None, g_np[1], None], [d_np[0][1] if f == 1 else None for f in range(8)], None, None, None, d_np[4])
        assert _all_same(numpy(second), want), family

        # inputs that do not require grad the second time get None, and a side nothing asks for is not launched
        calls = []
        real_hvp, real_jvp = capi.trajectory_tracking_hvp, capi.trajectory_tracking_jvp
        capi.trajectory_tracking_hvp = lambda *x: (calls.append(("hvp", x[15], x[16], x[17:20])), real_hvp(*x))[1]
        capi.trajectory_tracking_jvp = lambda *x: (calls.append(("jvp",)), real_jvp(*x))[1]
        try:
            some = {nm: ins_a[nm] if nm in ("pos1", "duration0") else ins_a[nm].detach() for nm in NAMES}
            fixed = {nm: x.detach() for nm, x in ins_b.items()}
            grads = torch.autograd.grad(_run(some, fixed, lo.detach(), hi.detach(), delay.detach(), 2), [some["pos1"], some["duration0"]],
                                        grad_outputs=[x.detach() for x in g], create_graph=True)
            torch.autograd.grad((grads[0] * u[1]).sum() + (grads[1] * u[6]).sum(), [some["pos1"], some["duration0"]])
            assert len(calls) == 1 and calls[0][0] == "hvp", calls
            assert [bool(x) for x in calls[0][1]] == [nm in ("pos1", "duration0") for nm in NAMES], calls      # side A: the two asked for
            assert not any(calls[0][2]) and not any(calls[0][3]), calls                                         # side B and the queries: nothing
            del calls[:]
            detached = {nm: x.detach() for nm, x in ins_a.items()}
            grads = torch.autograd.grad(_run(detached, fixed, lo.detach(), hi.detach(), delay, 2), [delay], grad_outputs=g, create_graph=True)
            got = torch.autograd.grad((grads[0] * u[18]).sum(), g)      # the delay alone requires grad on the other side: its result alone
            assert [c[0] for c in calls] == ["jvp", "hvp"] and not any(calls[1][1]) and not any(calls[1][2]), calls
            assert [bool(x) for x in calls[1][3]] == [False, False, True], calls
            assert _all_same(numpy(got), tc._tjvp(a, b, lo_np, hi_np, dl_np, None, None, None, None, d_np[4])), family
        finally:
            capi.trajectory_tracking_hvp, capi.trajectory_tracking_jvp = real_hvp, real_jvp

        # torch.autograd.functional.vhp is the double backward and gives the entry's bits (the matrix is symmetric: v^T H = H v), and
        # functional.hvp runs.  Nothing is asserted on hvp's numbers: torch forms it by the double-backward trick, the derivative of the
        # double backward in its own cotangent, which a once-differentiable backward does not offer -- torch then reports zeros
        point = tuple(x.detach() for x in (ins_a["pos1"], ins_b["pos1"], delay))
        w = g_np[1] ** 2

        def loss(pa1, pb1, dl):
            va = {nm: pa1 if nm == "pos1" else x.detach() for nm, x in ins_a.items()}
            vb = {nm: pb1 if nm == "pos1" else x.detach() for nm, x in ins_b.items()}
            return (_t(w) * torch.nan_to_num(_run(va, vb, lo.detach(), hi.detach(), dl, 2)[1])).sum()

        _, vH = torch.autograd.functional.vhp(loss, point, (u[1], u[9], u[18]))
        wz = np.where(np.isnan(first[1, "out"][1]), 0.0, w)
        want = _thvp(a, b, lo_np, hi_np, dl_np, [None, wz, None], [d_np[0][1] if f == 1 else None for f in range(8)],
                     [d_np[1][1] if f == 1 else None for f in range(8)], None, None, d_np[4])
        assert _all_same(numpy(vH), [want[1], want[9], want[18]]), family
        _, Hv = torch.autograd.functional.hvp(loss, point, (u[1], u[9], u[18]))
        assert [tuple(x.shape) for x in Hv] == [tuple(x.shape) for x in vH], family

        # against central differences of the device's first-order gradient along one direction of all nineteen inputs, d = max(|x|, 1) x a
        # standard normal, step e = 1e-6, over the queries the CPU rule keeps (tracking_ref.kept_for_differences), normwise per problem
        keep_np = kr.kept_for_differences(a, b, lo_np, hi_np, dl_np)
        share = keep_np.sum() / (~np.isnan(first[1, "out"][0])).sum()
        keep = _t(keep_np).bool()
        gk = [torch.where(keep, x.detach(), torch.zeros_like(x)) for x in g]
        s_np = hr.directions(a, b, lo_np, hi_np, dl_np, 2803, scaled=True)
        d = [_t(x) for x in s_np[0]] + [_t(x) for x in s_np[1]] + [torch.where(keep, _t(x), torch.zeros_like(lo)) for x in s_np[2:]]

        def gradient(sign):
            with torch.enable_grad():
                moved = [(x.detach() + sign * 1e-6 * dx).requires_grad_() for x, dx in zip(leaves, d)]
                return torch.autograd.grad(_run(dict(zip(NAMES, moved[:8])), dict(zip(NAMES, moved[8:16])), *moved[16:], 1), moved, grad_outputs=gk)

        fd = [((x - y) / 2e-6).cpu().numpy() for x, y in zip(gradient(+1), gradient(-1))]
        for at in (16, 17, 18):
            fd[at] = np.where(keep_np, fd[at], 0.0)
        grads = torch.autograd.grad(_run(ins_a, ins_b, lo, hi, delay, 2), leaves, grad_outputs=gk, create_graph=True)
        got = torch.autograd.grad(sum((gr_ * dx).sum() for gr_, dx in zip(grads, d)), leaves)
        err = tr.normwise(numpy(got), fd)[keep_np.any(axis=1)]
        print("%s: double backward against central differences of the device's gradient: worst %.2e normwise, %.0f %% of the finite queries kept"
              % (family, err.max(), 100 * share))
        assert share >= 0.5 and err.max() <= 1e-6, family

        # second order only, and order=1 not even that
        grads = torch.autograd.grad(_run(ins_a, ins_b, lo, hi, delay, 2), leaves, grad_outputs=gk, create_graph=True)
        (third,) = torch.autograd.grad((grads[5] ** 2).sum(), ins_a["duration0"], create_graph=True)
        for what, start in (("a third derivative", lambda: third.sum().backward()),
                            ("order=1's double backward", lambda: torch.autograd.grad(
                                (torch.nan_to_num(_run(ins_a, ins_b, lo, hi, delay, 1)[1]) ** 2).sum(), ins_a["vel1"], create_graph=True)[0].sum().backward())):
            try:
                start()
            except RuntimeError as e:
                assert "once_differentiable" in str(e), e
            else:
                raise AssertionError("%s did not raise" % what)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. end to end
def test_min_time_tracking_double_backward_against_the_chain_rule():
    """min_time_tracking(order=2), rest-to-rest, 300 golden problems against themselves 25 lower, delays U(0.02, 0.3) T, fixed windows: the
    double backward in both vehicles' positions of L = S w_o x output_o against the chain rule put together on the host from the device's
    own numbers.  Per vehicle, with z = (pos, x), x = (vel1, duration0, duration1) its solution, J and Hs the solution's Jacobian and second
    derivatives (min_time_hessian), z_bar the tracking integrals' gradient (the vjp entry), z_dot = (v, J v) for both vehicles and H z_dot
    the hvp entry along it: (the Hessian of L) v = [H z_dot]_pos + J^T [H z_dot]_x + S_a z_bar_{x_a} Hs[a] v."""
    n, k = N, 8
    pos = gg._golden_positions(n)
    p = [[pos[:, c] for c in range(3)], [pos[:, c] - 25.0 for c in range(3)]]
    xs = [[_t(x).requires_grad_() for x in side] for side in p]
    sols = [rp.min_time_hessian(*[x.detach() for x in side], gap_tol=1e-13) for side in xs]
    x0 = [[t.cpu().numpy() for t in s[:3]] for s in sols]
    status = [s[4].cpu().numpy() for s in sols]
    J, Hs = [s[5].cpu().numpy() for s in sols], [s[6].cpu().numpy() for s in sols]
    usable = np.ones(n, dtype=bool)
    for s in x0:
        usable &= np.isfinite(np.stack(s, 1)).all(1) & (s[1] > 0) & (s[2] > 0)
    zero = np.zeros(n)
    guess = [[side[0], side[1], side[2], zero, zero] + [np.where(usable, x, 1.0) for x in s] for side, s in zip(p, x0)]
    dl_np = gr.delays(guess[0], guess[1], k, 23, follow=True)      # fixed times: no part of the solutions
    lo_np, hi_np = gr.windows(guess[0], guess[1], dl_np, 24)
    rng = np.random.default_rng(25)
    w = [rng.uniform(0.5, 1.5, (n, k)) * s for s in (1.0, 0.1, 1.0)]
    v = [rng.standard_normal((n, 3)) for _ in range(2)]
    out = rp.min_time_tracking(xs[0], xs[1], _t(lo_np), _t(hi_np), _t(dl_np), gap_tol=1e-13, order=2)
    given = [[x.detach().cpu().numpy() for x in out[3 + side][:3]] for side in range(2)]      # the solutions the integrals were given
    loss = sum((_t(x) * torch.nan_to_num(o)).sum() for x, o in zip(w, out[:3]))               # an empty window's outputs are NaN and count as 0
    leaves = xs[0] + xs[1]
    grads = torch.autograd.grad(loss, leaves, create_graph=True)
    got = torch.autograd.grad(sum((gr_ * _t(v[c // 3][:, c % 3])).sum() for c, gr_ in enumerate(grads)), leaves)
    got = [np.stack([x.cpu().numpy() for x in got[3 * side:3 * side + 3]], axis=1) for side in range(2)]

    sp = [[side[0], side[1], side[2], zero, zero] + s for side, s in zip(p, given)]
    miss = np.isnan(out[0].detach().cpu().numpy())
    wz = [np.where(miss, 0.0, x) for x in w]
    z_bar = tc._tvjp(sp[0], sp[1], lo_np, hi_np, dl_np, wz, want_q=(False,) * 3)
    Jv = [np.einsum("nab,nb->na", J[side], v[side]) for side in range(2)]
    dots = [[v[side][:, 0], v[side][:, 1], v[side][:, 2], None, None, Jv[side][:, 0], Jv[side][:, 1], Jv[side][:, 2]] for side in range(2)]
    Hz = _thvp(sp[0], sp[1], lo_np, hi_np, dl_np, wz, dots[0], dots[1], None, None, None, want_q=(False,) * 3)
    fine = usable.copy()
    errs = []
    for side in range(2):
        Hz_s = Hz[8 * side:8 * side + 8]
        x_bar, Hz_x = np.stack(z_bar[side][5:8], axis=1), np.stack(Hz_s[5:8], axis=1)
        terms = np.concatenate([np.stack(Hz_s[:3], axis=1)[:, None, :], np.einsum("nab,na->nab", J[side], Hz_x),
                                np.einsum("na,nabc,nc->nacb", x_bar, Hs[side], v[side]).reshape(n, 9, 3)], axis=1).astype(LD)
        want, size = terms.sum(axis=1), np.abs(terms).sum(axis=1)
        fine &= ((status[side] & capi.ST_CONVERGED) != 0) & np.isfinite(got[side]).all(axis=1) & np.isfinite(np.asarray(size, dtype=np.float64)).all(axis=1)
        errs.append(np.asarray(np.abs(got[side] - want) / np.where(size > 0, size, LD(1)), dtype=np.float64).max(axis=1))
    err = np.maximum(errs[0], errs[1])
    good = fine & (err <= 1e-12)
    print("%d of %d pairs converged and finite; double backward against the chain rule: median %.2e, worst %.2e of the sum of |terms|; "
          "within 1e-12: %.1f %% of the pairs (asserted > 95 %%)" % (int(fine.sum()), n, np.median(err[fine]), err[fine].max(), 100 * good.mean()))
    assert good.mean() > 0.95

    # with end velocities that require grad the solve is first order: the double backward through it raises
    vel = (_t(zero[:64]).requires_grad_(), _t(zero[:64]))
    few = [[x[:64].detach().requires_grad_() for x in side] for side in xs]
    out = rp.min_time_tracking(few[0], few[1], _t(lo_np[:64]), _t(hi_np[:64]), _t(dl_np[:64]), vel_a=vel, gap_tol=1e-13, order=2)
    grads = torch.autograd.grad((torch.nan_to_num(out[1]) ** 2).sum(), few[0], create_graph=True)
    try:
        sum(x.sum() for x in grads).backward()
    except RuntimeError as e:
        assert "once_differentiable" in str(e), e
    else:
        raise AssertionError("a double backward through the solve with end velocities did not raise")
    torch.cuda.synchronize()


if __name__ == "__main__":
    globals()[sys.argv[1]](*sys.argv[2:])
    print("case ok")
