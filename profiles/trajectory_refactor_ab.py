"""A/B of the spline query kernels (csrc/trajectory.hip; DESIGN.md sections 13-17) between two builds of librp_batch.so, selected with
RP_BATCH_LIB: the same bits, the same speed.  Three modes, each a fresh process:

    python profiles/trajectory_refactor_ab.py bits OUT.npz       every entry's outputs on seeded inputs into one file
    python profiles/trajectory_refactor_ab.py compare A.npz B.npz   per-array SHA-1 of two such files; exit status 1 unless all are equal
    python profiles/trajectory_refactor_ab.py time               the median time of each entry at profiles/integrals_timing.py's two shapes

bits: rp_trajectory_eval, _vjp, _jvp, _hvp, rp_trajectory_crossing, rp_trajectory_extrema, rp_trajectory_integrals, _vjp, _jvp on
tests/trajectory_ref.py's random_states, with their end velocities and with NULL end velocities; rp_batch_trajectory_device,
rp_batch_crossing_device, rp_batch_extrema_device, rp_batch_integrals_device and rp_batch_sample_device on a solved F3 batch, given with end
velocities and without.  Shapes: 300,001 problems x 1 and 2 queries (more trips than the grid's cap, a partial last trip, an odd total), 1,031 x
7, 64, 67, 130 (a group of fewer than 64 lanes, exactly 64, more units than lanes for odd and for even k) and 5 x 4,096 (a trip of 2 problems
and of 1).  Each entry runs with everything wanted, then with each output, each upstream gradient, each window end, each per-query tangent
and each tangent table NULL in turn.

time: HIP events on the batch's stream, 3 warm-up and 20 timed repetitions per entry, everything wanted, the entries taking turns."""
import hashlib
import os
import sys

import numpy as np
import torch

torch.cuda.init()      # before the product library: tests/test_gpu_boundary.py

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "tests"))
import crossing_ref as cr  # noqa: E402
import end_velocity_ref as er  # noqa: E402
import extrema_ref as xr  # noqa: E402
import rocket_path_amd as rp  # noqa: E402
import trajectory_ref as tr  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

DEV = "cuda:0"
SHAPES = ((300001, 1), (300001, 2), (1031, 7), (1031, 64), (1031, 67), (1031, 130), (5, 4096))
REPS, WARMUP = 20, 3


def dev(a):
    if a is None:
        return None
    t = torch.as_tensor(np.ascontiguousarray(a, dtype=np.float64), device=DEV)
    torch.cuda.synchronize()      # the batch's stream does not wait for torch's null stream
    return t


def ptr(t):
    return t.data_ptr() if t is not None else 0


def fresh(*shape):
    t = torch.full(shape, 7.0, dtype=torch.float64, device=DEV)
    torch.cuda.synchronize()
    return t


class Recorder:
    def __init__(self):
        self.arrays = {}

    def run(self, name, launch, shapes, sync):
        """launch(addresses) with one fresh buffer per wanted shape (None: not wanted, address 0); every buffer is kept under name/index."""
        outs = [fresh(*s) if s is not None else None for s in shapes]
        launch([ptr(o) for o in outs])
        sync()
        for j, o in enumerate(outs):
            if o is not None:
                self.arrays[("%s/%d" % (name, j)).replace("/", " | ")] = o.cpu().numpy()


def without(items, j):
    return [None if i == j else x for i, x in enumerate(items)]


def stateless(rec, tag, sp, n, k, seed, null_vel, variations):
    rng = np.random.default_rng(seed)
    ts = [dev(a) for a in sp]
    spline = [ptr(t) for t in ts]
    if null_vel:
        spline[3] = spline[4] = 0
    tau = dev(tr.query_times(sp, k, seed + 1))
    level = dev(cr.levels(sp, k, seed + 2))
    lo, hi = (dev(a) for a in xr.windows(sp, k, seed + 3))
    g = [dev(rng.standard_normal((n, k))) for _ in range(4)]
    dots = [dev(rng.standard_normal(n)) for _ in range(8)]
    tdot, lo_dot, hi_dot = (dev(rng.standard_normal((n, k))) for _ in range(3))
    nk, bars = [(n, k)], [(n,)] * 8
    sync = torch.cuda.synchronize

    def each(name, launch, inputs, shapes):
        """Everything given and wanted; then (variations) each input and each output left out in turn."""
        rec.run("%s/%s/all" % (tag, name), lambda out: launch(inputs, out), shapes, sync)
        if not variations:
            return
        for j in range(len(inputs)):
            rec.run("%s/%s/no input %d" % (tag, name, j), lambda out: launch(without(inputs, j), out), shapes, sync)
        if len(shapes) > 1:
            for j in range(len(shapes)):
                rec.run("%s/%s/no output %d" % (tag, name, j), lambda out: launch(inputs, out), without(shapes, j), sync)

    def table(xs):
        return [ptr(x) for x in xs] if xs is not None else None

    each("eval", lambda i, o: capi.trajectory_eval(0, 0, n, k, spline, ptr(tau), *o), [], nk * 3)
    each("vjp", lambda i, o: capi.trajectory_eval_vjp(0, 0, n, k, spline, ptr(tau), ptr(i[0]), ptr(i[1]), ptr(i[2]), o[:8], o[8]), g[:3], bars + nk)
    each("jvp", lambda i, o: capi.trajectory_eval_jvp(0, 0, n, k, spline, ptr(tau), table(i[0]), ptr(i[1]), *o), [dots, tdot], nk * 3)
    each("hvp", lambda i, o: capi.trajectory_eval_hvp(0, 0, n, k, spline, ptr(tau), ptr(i[0]), ptr(i[1]), ptr(i[2]), table(i[3]), ptr(i[4]), o[:8], o[8]),
         g[:3] + [dots, tdot], bars + nk)
    rec.run("%s/crossing/all" % tag, lambda o: capi.trajectory_crossing(0, 0, n, k, spline, ptr(level), o[0], o[1]), nk * 2, sync)
    if variations:
        rec.run("%s/crossing/no output 1" % tag, lambda o: capi.trajectory_crossing(0, 0, n, k, spline, ptr(level), o[0], o[1]), nk + [None], sync)
    each("extrema", lambda i, o: capi.trajectory_extrema(0, 0, n, k, spline, ptr(i[0]), ptr(i[1]), o[:4], o[4:]), [lo, hi], nk * 8)
    each("integrals", lambda i, o: capi.trajectory_integrals(0, 0, n, k, spline, ptr(i[0]), ptr(i[1]), o), [lo, hi], nk * 4)
    each("integrals vjp", lambda i, o: capi.trajectory_integrals_vjp(0, 0, n, k, spline, ptr(i[0]), ptr(i[1]), table(i[2:6]), o[:8], o[8], o[9]),
         [lo, hi] + g, bars + nk * 2)
    each("integrals jvp", lambda i, o: capi.trajectory_integrals_jvp(0, 0, n, k, spline, ptr(i[0]), ptr(i[1]), table(i[2]), ptr(i[3]), ptr(i[4]), o),
         [lo, hi, dots, lo_dot, hi_dot], nk * 4)


def problems(n, seed, with_vel):
    p = rp.problems.generate(seed, 0, n, rp.problems.DIST_MONOTONE)
    if not with_vel:
        return list(p)
    rng = np.random.default_rng(seed)
    v0 = 0.1 * rng.uniform(-1, 1, n) * np.sqrt(er.L_DEFAULT * np.abs(p[1] - p[0]))
    v2 = 0.1 * rng.uniform(-1, 1, n) * np.sqrt(er.L_DEFAULT * np.abs(p[2] - p[1]))
    return list(p) + [v0, v2]


def on_batch(rec, tag, n, k, seed, with_vel, variations):
    args = [dev(a) for a in problems(n, seed, with_vel)]
    with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64) as b:
        if with_vel:
            b.set_problems_vel_device(*[ptr(t) for t in args])
        else:
            b.set_problems_device(*[ptr(t) for t in args])
        b.solve(1e-8, 200, 0)
        sp = tr.spline_of_state(b.get_state())
        rec.arrays["%s | state" % tag] = np.stack(sp)
        # the queries are drawn around a spline with usable durations everywhere; the kernels see the batch's own
        sp = [np.where(np.isfinite(a), a, 1.0) for a in sp]
        sp[6], sp[7] = (np.where(a > 0, a, 1.0) for a in (sp[6], sp[7]))
        tau, level = dev(tr.query_times(sp, k, seed + 1)), dev(cr.levels(sp, k, seed + 2))
        lo, hi = (dev(a) for a in xr.windows(sp, k, seed + 3))
        nk = [(n, k)]
        rec.run("%s/sample" % tag, lambda o: b.sample_device(o[0], o[1]), [(n, 66), (n, 4)], b.sync)
        runs = [("trajectory", lambda w, o: b.trajectory_device(ptr(tau), k, *o), nk * 3, 0),
                ("crossing", lambda w, o: b.crossing_device(ptr(level), k, o[0], o[1]), nk * 2, 0),
                ("extrema", lambda w, o: b.extrema_device(ptr(w[0]), ptr(w[1]), k, o[:4], o[4:]), nk * 8, 2),
                ("integrals", lambda w, o: b.integrals_device(ptr(w[0]), ptr(w[1]), k, o), nk * 4, 2)]
        for name, launch, shapes, ends in runs:
            rec.run("%s/%s/all" % (tag, name), lambda o: launch([lo, hi], o), shapes, b.sync)
            if not variations:
                continue
            for j in range(ends):
                rec.run("%s/%s/no input %d" % (tag, name, j), lambda o: launch(without([lo, hi], j), o), shapes, b.sync)
            for j in range(len(shapes)):
                if name != "crossing" or j == 1:      # the crossing times cannot be left out
                    rec.run("%s/%s/no output %d" % (tag, name, j), lambda o: launch([lo, hi], o), without(shapes, j), b.sync)


def bits(path):
    rec = Recorder()
    for n, k in SHAPES:
        seed = 1000 * k + n % 1000
        stateless(rec, "%dx%d" % (n, k), tr.random_states(n, seed), n, k, seed, False, True)
        stateless(rec, "%dx%d null vel" % (n, k), tr.random_states(n, seed), n, k, seed, True, False)
        on_batch(rec, "%dx%d batch vel" % (n, k), n, k, seed, True, True)
        on_batch(rec, "%dx%d batch" % (n, k), n, k, seed, False, False)
        print("%d x %d done: %d arrays so far" % (n, k, len(rec.arrays)), flush=True)
    np.savez(path, **rec.arrays)
    print("%d arrays, %d bytes -> %s" % (len(rec.arrays), sum(a.nbytes for a in rec.arrays.values()), path))


def compare(path_a, path_b):
    a, b = np.load(path_a), np.load(path_b)
    digest = lambda x: hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()      # noqa: E731
    differing = sorted(set(a.files) ^ set(b.files))
    total = 0
    for name in sorted(set(a.files) & set(b.files)):
        x, y = a[name], b[name]
        total += x.nbytes
        if x.shape != y.shape or digest(x) != digest(y):
            differing.append(name)
    print("%d / %d arrays, %d bytes a side, %d arrays differ" % (len(a.files), len(b.files), total, len(differing)))
    for name in differing[:40]:
        print("  differs: %s" % name)
    return 1 if differing else 0


def timing():
    print("device: %s, library: %s" % (torch.cuda.get_device_name(0), os.environ.get("RP_BATCH_LIB", "the tree's own")))
    for n, k in ((1 << 20, 64), (65536, 256)):
        torch.manual_seed(n + k)
        p = [torch.as_tensor(x, device=DEV) for x in rp.problems.generate(12345, 0, n, rp.problems.DIST_MONOTONE)]
        sol = torch.empty((n, 4), dtype=torch.float64, device=DEV)
        outs = [torch.empty((n, k), dtype=torch.float64, device=DEV) for _ in range(8)]
        g = [torch.randn((n, k), dtype=torch.float64, device=DEV) for _ in range(4)]
        bars = [torch.empty(n, dtype=torch.float64, device=DEV) for _ in range(8)]
        dots = [torch.randn(n, dtype=torch.float64, device=DEV) for _ in range(8)]
        torch.cuda.synchronize()
        with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            b.set_problems_device(*[x.data_ptr() for x in p])
            b.solve(1e-8, 200, 0)
            b.solution_device(sol.data_ptr())
            b.sync()
            vel1, d0, d1 = (sol[:, c].contiguous() for c in range(3))
            T = (d0 + d1).unsqueeze(1)
            lo = ((torch.rand((n, k), dtype=torch.float64, device=DEV) * 1.2 - 0.1) * T).contiguous()
            hi = ((torch.rand((n, k), dtype=torch.float64, device=DEV) * 1.2 - 0.1) * T).contiguous()
            lo, hi = torch.minimum(lo, hi), torch.maximum(lo, hi)
            level = (p[0].unsqueeze(1) + torch.rand((n, k), dtype=torch.float64, device=DEV) * (p[2] - p[0]).unsqueeze(1)).contiguous()
            torch.cuda.synchronize()
            spline = [p[0].data_ptr(), p[1].data_ptr(), p[2].data_ptr(), 0, 0, vel1.data_ptr(), d0.data_ptr(), d1.data_ptr()]
            o, gp = [x.data_ptr() for x in outs], [x.data_ptr() for x in g]
            bar, dot = [x.data_ptr() for x in bars], [x.data_ptr() for x in dots]
            tau, tdot, lp, hp, lv = lo.data_ptr(), g[3].data_ptr(), lo.data_ptr(), hi.data_ptr(), level.data_ptr()
            s = b.stream()
            pos66 = torch.empty((n, 66), dtype=torch.float64, device=DEV)
            torch.cuda.synchronize()
            launches = (
                ("rp_trajectory_eval", lambda: capi.trajectory_eval(0, s, n, k, spline, tau, o[0], o[1], o[2])),
                ("rp_trajectory_eval_vjp", lambda: capi.trajectory_eval_vjp(0, s, n, k, spline, tau, gp[0], gp[1], gp[2], bar, o[0])),
                ("rp_trajectory_eval_jvp", lambda: capi.trajectory_eval_jvp(0, s, n, k, spline, tau, dot, tdot, o[0], o[1], o[2])),
                ("rp_trajectory_eval_hvp", lambda: capi.trajectory_eval_hvp(0, s, n, k, spline, tau, gp[0], gp[1], gp[2], dot, tdot, bar, o[0])),
                ("rp_batch_trajectory_device", lambda: b.trajectory_device(tau, k, o[0], o[1], o[2])),
                ("rp_trajectory_crossing", lambda: capi.trajectory_crossing(0, s, n, k, spline, lv, o[0], o[1])),
                ("rp_batch_crossing_device", lambda: b.crossing_device(lv, k, o[0], o[1])),
                ("rp_trajectory_extrema", lambda: capi.trajectory_extrema(0, s, n, k, spline, lp, hp, o[:4], o[4:])),
                ("rp_batch_extrema_device", lambda: b.extrema_device(lp, hp, k, o[:4], o[4:])),
                ("rp_trajectory_integrals", lambda: capi.trajectory_integrals(0, s, n, k, spline, lp, hp, o[:4])),
                ("rp_trajectory_integrals_vjp", lambda: capi.trajectory_integrals_vjp(0, s, n, k, spline, lp, hp, gp, bar, o[0], o[1])),
                ("rp_trajectory_integrals_jvp", lambda: capi.trajectory_integrals_jvp(0, s, n, k, spline, lp, hp, dot, gp[0], gp[1], o[:4])),
                ("rp_batch_integrals_device", lambda: b.integrals_device(lp, hp, k, o[:4])),
                ("rp_batch_sample_device", lambda: b.sample_device(pos66.data_ptr(), o[1])),
            )
            times = {name: [] for name, _ in launches}
            for r in range(WARMUP + REPS):
                for name, launch in launches:
                    b.event_record(0)
                    launch()
                    b.event_record(1)
                    b.sync()
                    if r >= WARMUP:
                        times[name].append(b.event_elapsed_ms(0, 1))
        for name, _ in launches:
            t = times[name]
            print("n %8d k %4d  %-28s median %9.4f ms  (min %9.4f, max %9.4f)" % (n, k, name, float(np.median(t)), min(t), max(t)), flush=True)
        del outs, g, lo, hi, level
        torch.cuda.empty_cache()


if __name__ == "__main__":
    mode = sys.argv[1] if len(sys.argv) > 1 else ""
    if mode == "bits" and len(sys.argv) == 3:
        bits(sys.argv[2])
    elif mode == "compare" and len(sys.argv) == 4:
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    elif mode == "time" and len(sys.argv) == 2:
        timing()
    else:
        sys.exit(__doc__)
