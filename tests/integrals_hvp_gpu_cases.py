"""The cases of tests/test_gpu_integrals_hvp.py, each run in a fresh process (`python tests/integrals_hvp_gpu_cases.py <case> [family]`), on
top of tests/integrals_gpu_cases.py's helpers.  Not collected by pytest (no test_ prefix on the file).  What is checked, and why each
bound is what it is: DESIGN.md section 19."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import integrals_gpu_cases as ic  # noqa: E402  (initialises torch's HIP runtime first, and sets the paths)

import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.autograd.forward_ad as fwAD  # noqa: E402

import extrema_ref as xr  # noqa: E402
import integrals_hvp_ref as hr  # noqa: E402
import integrals_ref as ir  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

tg = ic.tg
BIG, NS, NAMES = ic.BIG, tg.NS, ic.NAMES
KS = (1, 2, 7, 8, 33, 64, 65, 200)      # every group size G, both pair paths, more units than lanes, a partial last trip
LD = np.longdouble
CPU_BOUND = 1e-12                        # tests/test_integrals_hvp_cpu.py's bound on the float64 restatement, normwise per problem
_t, _bits, _same_bits, _head, Out, _dev, _ptr, _all_same = ic._t, ic._bits, ic._same_bits, ic._head, ic.Out, ic._dev, ic._ptr, ic._all_same
_flat = hr.flat


def _ihvp(sp, lo, hi, g, dots, lo_dot, hi_dot, want_bars=(True,) * 8, want_lo=True, want_hi=True, k=None):
    """g: four (n, k) arrays or None each (NULL), or None (a NULL table); dots: eight arrays of n or None each, or None (a NULL table);
    lo_dot, hi_dot (n, k) or None.  Returns (eight bar_dots or None each, lo_bar_dot, hi_bar_dot)."""
    n = len(sp[0])
    k = k if k is not None else (lo if lo is not None else hi).shape[1]
    ts, addr = ic._addr(sp)
    tl, th, tld, thd = _dev(lo), _dev(hi), _dev(lo_dot), _dev(hi_dot)
    gs = [_dev(x) for x in g] if g is not None else None
    ds = [_dev(x) for x in dots] if dots is not None else None
    bars = [Out(n) if w else None for w in want_bars]
    lb, hb = Out(n, k) if want_lo else None, Out(n, k) if want_hi else None
    capi.trajectory_integrals_hvp(0, 0, n, k, addr, _ptr(tl), _ptr(th), [_ptr(x) for x in gs] if gs is not None else None,
                                  [_ptr(x) for x in ds] if ds is not None else None, _ptr(tld), _ptr(thd), [o.ptr if o else 0 for o in bars],
                                  lb.ptr if lb else 0, hb.ptr if hb else 0)
    torch.cuda.synchronize()
    return [o.get() if o else None for o in bars], lb.get() if lb else None, hb.get() if hb else None


def _normwise(a, b):
    """The worst of trajectory_ref.normwise over the problems -- where a problem's reference is exactly 0, the norm of the difference
    itself -- and never a NaN."""
    a = np.concatenate([np.asarray(x, dtype=LD).reshape(len(x), -1) for x in a], axis=1)
    b = np.concatenate([np.asarray(x, dtype=LD).reshape(len(x), -1) for x in b], axis=1)
    miss, size = np.linalg.norm((a - b).astype(np.float64), axis=1), np.linalg.norm(b.astype(np.float64), axis=1)
    worst = float(np.max(miss / np.where(size > 0, size, 1.0)))
    assert np.isfinite(worst), "a NaN or infinite result"
    return worst


def _rows(x, n):
    return [a[:n] for a in x]


def _inputs(family, sp, k, seed):
    """Windows (short ones from the fourth column on; column 0 is the whole spline), gradients on all four outputs and a direction in all
    ten inputs -- on the rest-to-rest family one that keeps the end velocities (integrals_hvp_ref.keeps_the_end_velocities: along the
    others the distance's second derivative is one-sided at the spline's own ends, and two precisions may take different sides)."""
    lo, hi = ic._windows(family, sp, k, seed)
    g = hr.gradients(lo.shape, seed + 1)
    dots, lo_dot, hi_dot = hr.directions(sp, lo, seed + 2)
    if family == "rest":
        dots = hr.keeps_the_end_velocities(dots)
    return lo, hi, g, dots, lo_dot, hi_dot


# ---------------------------------------------------------------- 1. the entry against longdouble
def test_entry_against_longdouble_nulls_and_nan_rule(family):
    """Normwise per problem against the longdouble definition: the float64 restatement of the kernel's arithmetic and order first, on the
    same inputs on the CPU; the device is held to 10 x the restatement's worst (DESIGN.md section 12's margin).  The reference is formed for
    4,097 problems at k <= 2, 1,025 at k = 7 and 8 and 257 beyond (it is the slow part), and the device runs every n up to that."""
    sp_all = ic._family(family)
    worst = [0.0, 0.0]      # [restatement, device]
    for k in KS:
        n_ref = min(len(sp_all[0]), BIG if k <= 2 else (1025 if k <= 8 else 257))
        sp_ref = _head(sp_all, n_ref)
        lo_r, hi_r, g_r, dots_r, ld_r, hd_r = _inputs(family, sp_ref, k, 1300 + k)
        want = _flat(hr.hvp_ld(sp_ref, lo_r, hi_r, g_r, dots_r, ld_r, hd_r))
        worst[0] = max(worst[0], _normwise(_flat(hr.hvp_f64(sp_ref, lo_r, hi_r, g_r, dots_r, ld_r, hd_r)), want))
        for n in sorted(set(m for m in NS if m < n_ref) | {n_ref}):
            sp, lo, hi, g, dots, lo_dot, hi_dot = _head(sp_ref, n), lo_r[:n], hi_r[:n], _rows(g_r, n), _rows(dots_r, n), ld_r[:n], hd_r[:n]
            full = _ihvp(sp, lo, hi, g, dots, lo_dot, hi_dot)
            worst[1] = max(worst[1], _normwise(_flat(full), _rows(want, n)))
            if n != min(65, n_ref) or k not in (7, 8):
                continue
            # every NULL input against explicit zeros: the same bits
            z, zn = np.zeros((n, k)), np.zeros(n)
            for f in range(4):
                a = _ihvp(sp, lo, hi, [None if j == f else x for j, x in enumerate(g)], dots, lo_dot, hi_dot)
                e = _ihvp(sp, lo, hi, [z if j == f else x for j, x in enumerate(g)], dots, lo_dot, hi_dot)
                assert _all_same(_flat(a), _flat(e)), (family, k, "g", f)
            assert _all_same(_flat(_ihvp(sp, lo, hi, None, dots, lo_dot, hi_dot)), _flat(_ihvp(sp, lo, hi, [z] * 4, dots, lo_dot, hi_dot))), (family, k)
            for null in ((True,) * 8, (True, False) * 4, (False, True) * 4):
                a = _ihvp(sp, lo, hi, g, [None if m else x for x, m in zip(dots, null)], lo_dot, hi_dot)
                e = _ihvp(sp, lo, hi, g, [zn if m else x for x, m in zip(dots, null)], lo_dot, hi_dot)
                assert _all_same(_flat(a), _flat(e)), (family, k, null)
            assert _all_same(_flat(_ihvp(sp, lo, hi, g, None, lo_dot, hi_dot)), _flat(_ihvp(sp, lo, hi, g, [zn] * 8, lo_dot, hi_dot))), (family, k)
            for ld_null, hd_null in ((True, False), (False, True), (True, True)):
                a = _ihvp(sp, lo, hi, g, dots, None if ld_null else lo_dot, None if hd_null else hi_dot)
                e = _ihvp(sp, lo, hi, g, dots, z if ld_null else lo_dot, z if hd_null else hi_dot)
                assert _all_same(_flat(a), _flat(e)), (family, k, ld_null, hd_null)
            # every output alone and alone left out: only what is asked for is written (Out.get checks the sentinels), with the full call's bits
            for f in range(10):
                for alone in (True, False):
                    wanted = [(j == f) == alone for j in range(10)]
                    some = _flat(_ihvp(sp, lo, hi, g, dots, lo_dot, hi_dot, want_bars=wanted[:8], want_lo=wanted[8], want_hi=wanted[9]))
                    for j, x in enumerate(some):
                        assert (x is None) == (not wanted[j]) and (x is None or _same_bits(x, _flat(full)[j])), (family, k, f, alone, j)
    print("%s: hvp against longdouble, normwise: the float64 restatement %.2e, the device %.2e, asserted %.2e" % (family, worst[0], worst[1], 10 * worst[0]))
    assert worst[1] <= 10 * worst[0], family
    if family == "knot":
        return
    # the NaN rule: a duration of 0, -1, inf, NaN poisons its problem's eight results and no other problem; a query whose outputs are NaN
    # (its problem's, a NaN or an empty window) counts with gradients of zero and gets lo_bar_dot = hi_bar_dot = 0; a NaN lo_dot on an end
    # that is taken makes its own lo_bar_dot and its problem's sums NaN
    m, k = 257, 7
    sp = [a.copy() for a in _head(sp_all, m)]
    lo, hi = xr.windows(sp, k, 1)
    g = hr.gradients(lo.shape, 2)
    dots, lo_dot, hi_dot = hr.directions(sp, lo, 3)
    clean = _ihvp(sp, lo, hi, g, dots, lo_dot, hi_dot)
    assert all(np.isfinite(x).all() for x in _flat(clean))
    sp[6][3], sp[7][64], sp[6][130], sp[7][256] = 0.0, np.inf, -1.0, np.nan
    lo[10, 0], hi[200, 4], lo[11, 3], hi[11, 3] = np.nan, np.nan, np.inf, np.inf
    T = sp[6] + sp[7]
    lo[50, 2], hi[50, 2] = 0.25 * sp[6][50], 0.75 * sp[6][50]      # inside segment 0, both ends taken
    lo_dot[50, 2] = np.nan
    bad_rows = np.zeros(m, dtype=bool)
    bad_rows[[3, 64, 130, 256]] = True
    empty = np.isnan(ir.integrals_f64(sp, lo, hi)[0])
    assert empty[bad_rows].all() and empty[10, 0] and empty[200, 4] and empty[11, 3] and not empty[50, 2] and T[50] > 0
    bars, lb, hb = _ihvp(sp, lo, hi, g, dots, lo_dot, hi_dot)
    assert np.all(lb[empty] == 0) and np.all(hb[empty] == 0), family
    nan_lb = np.isnan(lb)
    assert nan_lb[50, 2] and nan_lb.sum() == 1 and not np.isnan(hb).any(), family
    touched = [3, 64, 130, 256, 10, 200, 11, 50]
    rest = np.delete(np.arange(m), touched)
    for f, b in enumerate(bars):
        assert np.isnan(b[bad_rows]).all(), (family, f)
        assert np.isfinite(b[[10, 200, 11]]).all(), (family, f)
        assert np.isnan(b[50]) == (f not in (2, 4, 7)), (family, f)      # segment 0's sums reach everything but pos2, vel2, duration1
        assert np.array_equal(_bits(b[rest]), _bits(clean[0][f][rest])), (family, f)
    for x, c in ((lb, clean[1]), (hb, clean[2])):
        assert np.array_equal(_bits(x[rest]), _bits(c[rest])), family


# ---------------------------------------------------------------- 2. reproducibility
def test_bits_depend_on_the_problem_and_k_only():
    roll = lambda x: np.concatenate([x[1:], x[:1]])      # noqa: E731
    for family in ("solved", "random", "rest"):
        sp = ic._family(family)
        for k in KS:
            lo, hi, g, dots, lo_dot, hi_dot = _inputs(family, sp, k, 1500 + k)
            big = _flat(_ihvp(sp, lo, hi, g, dots, lo_dot, hi_dot))
            assert _all_same(big, _flat(_ihvp(sp, lo, hi, g, dots, lo_dot, hi_dot))), (family, k, "differs from run to run")
            for n in NS[:-1]:
                small = _flat(_ihvp(_head(sp, n), lo[:n], hi[:n], _rows(g, n), _rows(dots, n), lo_dot[:n], hi_dot[:n]))
                assert _all_same(small, _rows(big, n)), (family, n, k)
            moved = _flat(_ihvp([roll(a) for a in sp], roll(lo), roll(hi), [roll(x) for x in g], [roll(x) for x in dots], roll(lo_dot), roll(hi_dot)))
            for a, b in zip(moved, big):      # problem 0 moved to the end
                assert _same_bits(a[-1], b[0]) and _same_bits(a[:-1], b[1:]), (family, k)
    # more trips than the grid's cap: 300,001 problems of one window each are 2,344 trips of 128 for 2,048 blocks
    n = tg.GRID_N
    sp = tr.random_states(n, 77)
    lo, hi = (x[:, 2:3].copy() for x in xr.windows(sp, 3, 78))
    g = hr.gradients(lo.shape, 79)
    dots, lo_dot, hi_dot = hr.directions(sp, lo, 80)
    got = _flat(_ihvp(sp, lo, hi, g, dots, lo_dot, hi_dot))
    f64 = _flat(hr.hvp_f64(sp, lo, hi, g, dots, lo_dot, hi_dot))
    err = _normwise(got, f64)      # a problem whose one window is empty has ten results of exactly 0
    same = sum(int((_bits(a) != _bits(b)).sum()) for a, b in zip(got, f64))
    print("%d problems x 1 window against the float64 restatement, normwise: worst %.2e, %d values not bit for bit; asserted %.0e" % (n, err, same, CPU_BOUND))
    assert err <= CPU_BOUND


# ---------------------------------------------------------------- 3. identities on the device
def test_symmetry_and_linearity_on_the_device():
    worst_sym = worst_lin = worst_one = 0.0
    for family in ("solved", "random", "rest"):
        sp_all = ic._family(family)
        for k in KS:
            n = 257 if k > 8 else 1025
            sp = _head(sp_all, n)
            lo, hi = ic._windows(family, sp, k, 1700 + k)
            g = hr.gradients(lo.shape, 1701 + k)
            u, v = hr.directions(sp, lo, 1702 + k), hr.directions(sp, lo, 1703 + k)
            # u^T H[g] v = v^T H[g] u: both sides hold to the ~1e-14 normwise of the check against longdouble, so their difference to a few
            # times that of the sum of |terms| for these random directions: 1e-12, section 17's bound for the same identity
            left, size_l = hr.bilinear(_ihvp(sp, lo, hi, g, *v), u)
            right, size_r = hr.bilinear(_ihvp(sp, lo, hi, g, *u), v)
            sym = np.asarray(np.abs(left - right) / (size_l + size_r), dtype=np.float64)
            assert np.isfinite(sym).all(), (family, k)
            worst_sym = max(worst_sym, float(sym.max()))
            # linear in g: every gradient alone (the other three NULL), summed, is all four -- of the sum of |terms| over everything the
            # problem owns, as the symmetry above and every normwise check: a single result of the chain rule is a difference of terms that
            # can be thousands of times its size (a short segment), and taken alone it carries their rounding (printed beside it)
            every = _flat(_ihvp(sp, lo, hi, g, *v))
            alone = [_flat(_ihvp(sp, lo, hi, [x if j == f else None for j, x in enumerate(g)], *v)) for f in range(4)]
            miss_all, size_all = LD(0), LD(0)
            for j, c in enumerate(every):
                parts = [a[j].astype(LD) for a in alone]
                size = (sum(np.abs(x) for x in parts) + np.abs(c)).reshape(n, -1).sum(axis=1)
                miss = np.abs(sum(parts) - c.astype(LD)).reshape(n, -1).sum(axis=1)
                miss_all, size_all = miss_all + miss, size_all + size
                worst_one = max(worst_one, float(np.max(miss / np.where(size > 0, size, LD(1)))))
            lin = np.asarray(miss_all / np.where(size_all > 0, size_all, LD(1)), dtype=np.float64)
            assert np.isfinite(lin).all(), (family, k)
            worst_lin = max(worst_lin, float(lin.max()))
    print("symmetry %.2e, linearity in g %.2e of the sum of |terms| per problem (one result alone: %.2e); asserted 1e-12 each" % (worst_sym, worst_lin, worst_one))
    assert worst_sym <= 1e-12 and worst_lin <= 1e-12


# ---------------------------------------------------------------- 4. autograd
def _run(v, lo, hi, order):
    return rp.trajectory_integrals(v["pos0"], v["pos1"], v["pos2"], v["vel1"], v["duration0"], v["duration1"], lo, hi, vel0=v["vel0"], vel2=v["vel2"],
                                   order=order)


def test_autograd_order_2():
    n, k = 1025, 7
    for family in ("solved", "random", "rest"):
        sp = _head(ic._family(family), n)
        lo_np, hi_np = xr.windows(sp, k, 8)
        g_np = hr.gradients(lo_np.shape, 9)
        dots, lo_dot, hi_dot = hr.directions(sp, lo_np, 10)
        ins = {nm: _t(a).requires_grad_() for nm, a in zip(NAMES, sp)}
        lo, hi = _t(lo_np).requires_grad_(), _t(hi_np).requires_grad_()
        leaves = [ins[nm] for nm in NAMES] + [lo, hi]
        g = [_t(x).requires_grad_() for x in g_np]
        u = [_t(x) for x in dots] + [_t(lo_dot), _t(hi_dot)]

        # forward, backward (create_graph False and True) and forward mode: order=1's bits
        first = {}
        for order in (1, 2):
            outs = _run(ins, lo, hi, order)
            first[order, "out"] = [o.detach().cpu().numpy() for o in outs]
            for create_graph in (False, True):
                if order == 1 and create_graph:
                    continue
                grads = torch.autograd.grad(outs, leaves, grad_outputs=[x.detach() for x in g], create_graph=create_graph, retain_graph=True)
                first[order, create_graph] = [x.detach().cpu().numpy() for x in grads]
            only = torch.autograd.grad((g[3].detach() * torch.nan_to_num(_run(ins, lo, hi, order)[3])).sum(), leaves)      # three gradients go in as NULL
            first[order, "only"] = [x.cpu().numpy() for x in only]
            with fwAD.dual_level():
                dual = {nm: fwAD.make_dual(ins[nm].detach(), d) for nm, d in zip(NAMES, u[:8])}
                outs = _run(dual, fwAD.make_dual(lo.detach(), u[8]), fwAD.make_dual(hi.detach(), u[9]), order)
                first[order, "jvp"] = [fwAD.unpack_dual(x).tangent.cpu().numpy() for x in outs]
        for key in ("out", False, "only", "jvp"):
            assert _all_same(first[1, key], first[2, key]), (family, key)
        assert _all_same(first[1, False], first[2, True]), family
        assert _all_same(first[2, True], _flat(ic._ivjp(sp, lo_np, hi_np, g_np))), family

        # the double backward of a scalar loss: in the spline inputs and the window's ends the hvp entry, in the first backward's grad_outputs
        # the jvp entry (NaN where the output is: an empty window)
        grads = torch.autograd.grad(_run(ins, lo, hi, 2), leaves, grad_outputs=g, create_graph=True)
        s = sum((gr * x).sum() for gr, x in zip(grads, u))
        second = torch.autograd.grad(s, leaves + g, retain_graph=True)
        want = _flat(_ihvp(sp, lo_np, hi_np, g_np, dots, lo_dot, hi_dot)) + ic._ijvp(sp, lo_np, hi_np, dots, lo_dot, hi_dot)
        assert _all_same([a.cpu().numpy() for a in second], want), family
        # a loss on acc_sq alone, differentiated the second time along pos1 and hi alone: NULL gradients and NULL directions
        grads = torch.autograd.grad(_run(ins, lo, hi, 2)[3], [ins["pos1"], hi], grad_outputs=g[3].detach(), create_graph=True)
        s = (grads[0] * u[1]).sum() + (grads[1] * u[9]).sum()
        second = torch.autograd.grad(s, leaves)
        want = _flat(_ihvp(sp, lo_np, hi_np, [None, None, None, g_np[3]], [dots[1] if f == 1 else None for f in range(8)], None, hi_dot))
        assert _all_same([a.cpu().numpy() for a in second], want), family

        # inputs that do not require grad the second time get None, and a side nothing asks for is not launched
        calls = []
        real_hvp, real_jvp = capi.trajectory_integrals_hvp, capi.trajectory_integrals_jvp
        capi.trajectory_integrals_hvp = lambda *a: (calls.append(("hvp", a[11], a[12], a[13])), real_hvp(*a))[1]
        capi.trajectory_integrals_jvp = lambda *a: (calls.append(("jvp",)), real_jvp(*a))[1]
        try:
            some = {nm: ins[nm] if nm in ("pos1", "duration0") else ins[nm].detach() for nm in NAMES}
            grads = torch.autograd.grad(_run(some, lo.detach(), hi.detach(), 2), [some["pos1"], some["duration0"]], grad_outputs=[x.detach() for x in g],
                                        create_graph=True)
            torch.autograd.grad((grads[0] * u[1]).sum() + (grads[1] * u[6]).sum(), [some["pos1"], some["duration0"]])
            assert len(calls) == 1 and calls[0][0] == "hvp", calls
            assert [bool(a) for a in calls[0][1]] == [nm in ("pos1", "duration0") for nm in NAMES] and not calls[0][2] and not calls[0][3], calls
            del calls[:]
            grads = torch.autograd.grad(_run({nm: x.detach() for nm, x in ins.items()}, lo, hi.detach(), 2), [lo], grad_outputs=g, create_graph=True)
            got = torch.autograd.grad((grads[0] * u[8]).sum(), g)      # lo alone requires grad on the other side: of the hvp entry, lo's result alone
            assert [c[0] for c in calls] == ["jvp", "hvp"] and not any(calls[1][1]) and calls[1][2] and not calls[1][3], calls
            assert _all_same([a.cpu().numpy() for a in got], ic._ijvp(sp, lo_np, hi_np, [None] * 8, lo_dot, None)), family
        finally:
            capi.trajectory_integrals_hvp, capi.trajectory_integrals_jvp = real_hvp, real_jvp

        # against central differences of the device's first-order gradient along one direction of all ten inputs, d = max(|x|, 1) x a standard
        # normal, step e = 1e-6, over the queries the CPU rule keeps (tests/test_integrals_hvp_cpu.py), normwise per problem
        keep_np, _ = hr.kept_for_hvp_differences(sp, lo_np, hi_np)
        miss = np.isnan(first[1, "out"][0])
        share = keep_np.sum() / (~miss)[:, [0] + list(range(2, k))].sum()
        keep = _t(keep_np).bool()
        gk = [torch.where(keep, x.detach(), torch.zeros_like(x)) for x in g]
        d_np = hr.directions(sp, lo_np, 11, scaled=(lo_np, hi_np))
        d = [_t(x) for x in d_np[0]] + [torch.where(keep, _t(x), torch.zeros_like(lo)) for x in d_np[1:]]

        def gradient(sign):
            with torch.enable_grad():
                moved = [(x.detach() + sign * 1e-6 * dx).requires_grad_() for x, dx in zip(leaves, d)]
                return torch.autograd.grad(_run(dict(zip(NAMES, moved[:8])), moved[8], moved[9], 1), moved, grad_outputs=gk)

        fd = [((a - b) / 2e-6).cpu().numpy() for a, b in zip(gradient(+1), gradient(-1))]
        grads = torch.autograd.grad(_run(ins, lo, hi, 2), leaves, grad_outputs=gk, create_graph=True)
        got = torch.autograd.grad(sum((gr * dx).sum() for gr, dx in zip(grads, d)), leaves)
        err = tr.normwise([a.cpu().numpy() for a in got], fd)[keep_np.any(axis=1)]
        print("%s: double backward against central differences of the device's gradient: worst %.2e normwise, %.0f %% of the finite queries kept"
              % (family, err.max(), 100 * share))
        assert share >= 0.5 and err.max() <= 1e-6, family

        # second order only, and order=1 not even that
        grads = torch.autograd.grad(_run(ins, lo, hi, 2), leaves, grad_outputs=gk, create_graph=True)
        (third,) = torch.autograd.grad((grads[5] ** 2).sum(), ins["duration0"], create_graph=True)
        for what, start in (("a third derivative", lambda: third.sum().backward()),
                            ("order=1's double backward", lambda: torch.autograd.grad(
                                (torch.nan_to_num(_run(ins, lo, hi, 1)[2]) ** 2).sum(), ins["vel1"], create_graph=True)[0].sum().backward())):
            try:
                start()
            except RuntimeError as e:
                assert "once_differentiable" in str(e), e
            else:
                raise AssertionError("%s did not raise" % what)
    torch.cuda.synchronize()


# ---------------------------------------------------------------- 5. end to end
def test_min_time_integrals_double_backward_against_the_chain_rule():
    """min_time_integrals(order=2), rest-to-rest, the whole spline (column 0) and fixed windows: the double backward in the positions of
    L = S w_o x output_o against the chain rule put together on the host from the device's own numbers.  With z = (pos, x),
    x = (vel1, duration0, duration1) the solution, J and Hs its Jacobian and second derivatives (min_time_hessian), z_bar the integrals'
    gradient (the vjp entry), z_dot = (v, J v) and H z_dot the hvp entry along it:
    (the Hessian of L) v = [H z_dot]_pos + J^T [H z_dot]_x + S_a z_bar_{x_a} Hs[a] v."""
    n, k = 4096, 8
    p = rp.problems.generate(131, 0, n, rp.problems.DIST_REFERENCE_LIKE)
    pos = [_t(x).requires_grad_() for x in p]
    sol = rp.min_time_hessian(*[x.detach() for x in pos], gap_tol=1e-13)
    vel1, d0, d1 = (x.cpu().numpy() for x in sol[:3])
    status, J, Hs = sol[4].cpu().numpy(), sol[5].cpu().numpy(), sol[6].cpu().numpy()
    usable = np.isfinite(vel1) & np.isfinite(d0) & np.isfinite(d1) & (d0 > 0) & (d1 > 0)
    zero = np.zeros(n)
    spl = [p[0], p[1], p[2], zero, zero, np.where(usable, vel1, 0.0), np.where(usable, d0, 1.0), np.where(usable, d1, 1.0)]
    lo_np, hi_np = xr.windows(spl, k, 21)      # fixed times: no part of the solution
    rng = np.random.default_rng(22)
    w = [rng.uniform(0.5, 1.5, (n, k)) * s for s in (1.0, 1.0, 0.1, 0.01)]
    v = rng.standard_normal((n, 3))
    out = rp.min_time_integrals(*pos, _t(lo_np), _t(hi_np), gap_tol=1e-13, order=2)
    vel1, d0, d1 = (x.detach().cpu().numpy() for x in out[4:7])      # the solution the integrals were given
    loss = sum((_t(x) * torch.nan_to_num(o)).sum() for x, o in zip(w, out[:4]))      # an empty window's outputs are NaN and count as 0
    grads = torch.autograd.grad(loss, pos, create_graph=True)
    got = torch.autograd.grad(sum((gr * _t(v[:, c])).sum() for c, gr in enumerate(grads)), pos)
    got = np.stack([x.cpu().numpy() for x in got], axis=1)

    sp = [p[0], p[1], p[2], zero, zero, vel1, d0, d1]
    z_bar, _, _ = ic._ivjp(sp, lo_np, hi_np, w, want_lo=False, want_hi=False)
    Jv = np.einsum("nab,nb->na", J, v)
    Hz, _, _ = _ihvp(sp, lo_np, hi_np, w, [v[:, 0], v[:, 1], v[:, 2], None, None, Jv[:, 0], Jv[:, 1], Jv[:, 2]], None, None, want_lo=False, want_hi=False)
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
    out = rp.min_time_integrals(*few, _t(lo_np[:64]), _t(hi_np[:64]), vel0=vel0[:64], gap_tol=1e-13, order=2)
    grads = torch.autograd.grad((torch.nan_to_num(out[3]) ** 2).sum(), few, create_graph=True)
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
