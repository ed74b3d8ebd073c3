"""A/B of the torch layer of the fleet queries (rocket_path_amd/autograd.py; DESIGN.md sections 26-29) between two source trees that load
the same librp_batch.so: the same bits in every output, gradient and tangent, and the same host cost.  Modes, each a fresh process:

    python profiles/fleet_refactor_ab.py bits OUT.npz [TREE]      every output, reverse-mode gradient and forward-mode tangent into one file
    python profiles/fleet_refactor_ab.py compare A.npz B.npz      per-array SHA-1 of two such files; exit status 1 unless all are equal
    python profiles/fleet_refactor_ab.py time PARENT_TREE [NEW_TREE]   forward + backward of the four functions, the trees alternating
    python profiles/fleet_refactor_ab.py time-one [TREE]          one side's medians (what `time` starts, each with its own time limit)

TREE is the directory that holds rocket_path_amd (default: the one this file is in).  Another tree than this one has no build of its
own: RP_BATCH_LIB then defaults to this tree's library, so both sides run the same device code.

bits: trajectory_fleet_separation, trajectory_fleet_contact (start=None and start given: the four Functions), min_time_fleet_separation
and min_time_fleet_contact, d = 2 and 3, n = 3 scenes of m = 2, 3 and 7 vehicles, k = 1 and 4; windows given and with lo or hi None; the
level per scene and per pair; vehicle 0 of scene 1 with a NaN duration; scenes 2 and 0 built so that one vehicle of pair (0, 1) closes in on
the other, which rests, until its own end (the classes END of the second and of the first) and the first window of every scene of zero
width (the class LO); the other windows are narrow, so that a minimum sits on either end.  How many times fall into each class is
printed.  Seed fixed.

time: n = 3, m = 7, k = 4, d = 3, everything requiring a gradient; per function the median wall-clock time, host synchronised, of
forward plus backward.  `time` runs time-one ROUNDS times a side, parent first, and prints per function both sides' medians over the
rounds, the parent's own spread (its slowest round over its fastest) and whether the new median is within that spread of the parent's."""
import hashlib
import json
import os
import subprocess
import sys
import time as clock

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
DEV = "cuda:0"
ROUNDS, REPS, WARMUP, LIMIT = 6, 200, 20, 300


def load(tree):
    """torch (its HIP runtime first: tests/test_gpu_boundary.py) and the package of `tree`"""
    tree = os.path.abspath(tree or ROOT)
    if tree != ROOT:
        os.environ.setdefault("RP_BATCH_LIB", os.path.join(ROOT, "rocket_path_amd", "lib", "librp_batch.so"))
    import torch
    torch.cuda.init()
    sys.path.insert(0, tree)
    import rocket_path_amd as rp
    assert os.path.dirname(os.path.dirname(os.path.abspath(rp.__file__))) == tree, rp.__file__
    return torch, rp


def make_fleet(torch, n, m, d, seed, end_velocities):
    """Six or eight (n, m, d) tensors: (pos0, pos1, pos2, vel1, duration0, duration1[, vel0, vel2])"""
    g = torch.Generator().manual_seed(seed)
    rand = lambda lo, hi: (lo + (hi - lo) * torch.rand((n, m, d), dtype=torch.float64, generator=g))      # noqa: E731
    pos0, pos1, pos2 = rand(-1, 1), rand(-1, 1), rand(-1, 1)
    vel1, dur0, dur1 = rand(-1, 1), rand(0.5, 1.5), rand(0.5, 1.5)
    fleet = [pos0, pos1, pos2, vel1, dur0, dur1] + ([rand(-0.3, 0.3), rand(-0.3, 0.3)] if end_velocities else [])
    dur0[1, 0, 0] = float("nan")      # exactly that vehicle's m - 1 pairs are NaN
    # scene 2: vehicle 0 rests at the origin, vehicle 1 comes straight at it and stops short: the closest approach is vehicle 1's end
    # scene 0: the same with the two vehicles exchanged: the end of the pair's first vehicle
    for t in fleet:
        t[2, :2] = 0.0
        t[0, :2] = 0.0
    for s, still, moving in ((2, 0, 1), (0, 1, 0)):
        pos0[s, moving], pos1[s, moving], pos2[s, moving] = 4.0, 3.0, 2.0
        vel1[s, moving] = -1.0
        dur0[s, still], dur1[s, still] = 1.5, 1.5
        dur0[s, moving], dur1[s, moving] = 1.0, 1.0
    return [t.to(DEV) for t in fleet]


def make_windows(torch, n, k, seed):
    g = torch.Generator().manual_seed(seed)
    lo = 1.2 * torch.rand((n, k), dtype=torch.float64, generator=g)
    hi = lo + 0.4 * torch.rand((n, k), dtype=torch.float64, generator=g)
    hi[:, 0] = lo[:, 0]      # a window of zero width: the time is lo
    if k > 1:
        lo[0, 1], hi[0, 1] = 0.5, 9.0      # scenes 0 and 2 beyond their vehicles' ends
        lo[2, 1], hi[2, 1] = 0.5, 9.0
    return lo.to(DEV), hi.to(DEV)


class Recorder:
    def __init__(self, torch):
        self.torch, self.arrays, self.classes = torch, {}, {}

    def keep(self, name, t):
        if t is not None:
            self.arrays[name.replace("/", " | ")] = t.detach().cpu().numpy()

    def count(self, what, mask):
        self.classes[what] = self.classes.get(what, 0) + int(mask.sum())

    def derivatives(self, name, function, inputs):
        """function(*inputs) -> a tuple of tensors, the first differentiable.  Keeps the outputs, the gradient of every input under a
        seeded cotangent and the tangent of the first output under seeded tangents on every input.  Returns the detached outputs."""
        torch = self.torch
        import torch.autograd.forward_ad as fwAD
        g = torch.Generator().manual_seed(len(self.arrays))
        seeded = lambda t: torch.randn(t.shape, dtype=torch.float64, generator=g).to(DEV)      # noqa: E731
        leaves = [t.detach().clone().requires_grad_(True) if t is not None else None for t in inputs]
        out = function(*leaves)
        for j, o in enumerate(out):
            self.keep("%s/out %d" % (name, j), o)
        given = [t for t in leaves if t is not None]
        grads = iter(torch.autograd.grad(out[0], given, grad_outputs=seeded(out[0]), allow_unused=True))
        for j, t in enumerate(leaves):
            if t is not None:
                self.keep("%s/bar %d" % (name, j), next(grads))
        with fwAD.dual_level():
            duals = [fwAD.make_dual(t.detach(), seeded(t)) if t is not None else None for t in inputs]
            self.keep("%s/dot" % name, fwAD.unpack_dual(function(*duals)[0]).tangent)
        return [o.detach() for o in out]


def windows_of(lo, hi):
    return (("lo hi", lo, hi), ("no lo", None, hi), ("no hi", lo, None))


def fleet_functions(rec, rp, tag, fleet, start, lo, hi, m):
    torch = rec.torch
    nf = len(fleet)
    first, second = (x.to(DEV) for x in torch.triu_indices(m, m, 1))
    total = (fleet[4] + fleet[5])      # (n, m, d): every axis' end
    for st_name, st in (("no start", None), ("start", start)):
        for w_name, wl, wh in windows_of(lo, hi):
            name = "%s/%s/%s" % (tag, st_name, w_name)

            def separation(*x):
                return rp.trajectory_fleet_separation(x[:nf], x[nf], x[nf + 1], start=x[nf + 2])
            value, time = rec.derivatives(name + "/separation", separation, list(fleet) + [wl, wh, st])
            # the classes of the returned times: exact without a start; with one the scene-clock time is compared within 1e-12
            same = (lambda x, y: x == y) if st is None else (lambda x, y: torch.isclose(x, y, rtol=0.0, atol=1e-12))
            s_i = st[:, first].unsqueeze(2) if st is not None else torch.zeros_like(value[:, :, :1])
            delay = (st[:, second] - st[:, first]).unsqueeze(2) if st is not None else torch.zeros_like(value[:, :, :1])
            ok = ~torch.isnan(value)
            at_lo = same(time, wl.unsqueeze(1)) if wl is not None else ~ok
            at_hi = same(time, wh.unsqueeze(1)) if wh is not None else ~ok
            end_first = same(time.unsqueeze(3), (s_i + total[:, first]).unsqueeze(2)).any(dim=3)
            end_second = same(time.unsqueeze(3), (s_i + (delay + total[:, second])).unsqueeze(2)).any(dim=3)
            free = ok & ~at_lo & ~at_hi
            for what, mask in (("LO", ok & at_lo), ("HI", ok & at_hi & ~at_lo), ("END of the first", free & end_first),
                               ("END of the second", free & end_second & ~end_first),
                               ("START", free & same(time, s_i + delay) & (delay > 0)), ("missing", ~ok), ("queries", torch.ones_like(ok))):
                rec.count(what, mask)
        # a level that the pair reaches where its distance is not constant over the window: half way between f(lo) and the least f
        with torch.no_grad():
            f_lo = rp.trajectory_fleet_separation(fleet, lo, lo, start=st)[0]
            f_min = rp.trajectory_fleet_separation(fleet, lo, hi, start=st)[0]
            per_pair = 0.5 * (f_lo + f_min)
            per_pair = torch.where(torch.isnan(per_pair), torch.ones_like(per_pair), per_pair)
            levels = (("level per scene", per_pair.mean(dim=1)), ("level per pair", per_pair))
        for l_name, level in levels:
            for w_name, wl, wh in windows_of(lo, hi):
                name = "%s/%s/%s/%s" % (tag, st_name, l_name, w_name)

                def contact(*x):
                    return (rp.trajectory_fleet_contact(x[:nf], None, x[nf + 1], x[nf + 2], level_sq=x[nf], start=x[nf + 3]),)
                t, = rec.derivatives(name + "/contact", contact, list(fleet) + [level, wl, wh, st])
                rec.count("contacts", ~torch.isnan(t))
                rec.count("contact queries", torch.ones_like(t, dtype=torch.bool))


def pipelines(rec, rp, tag, n, m, d, k, seed, start, lo, hi):
    torch = rec.torch
    p = [torch.as_tensor(x).reshape(n, m, d).to(DEV) for x in rp.problems.generate(seed, 0, n * m * d, rp.problems.DIST_MONOTONE)]
    shift = torch.arange(m, dtype=torch.float64, device=DEV).reshape(1, m, 1) * 0.25      # the vehicles side by side, not on one point
    p = [x + shift for x in p]
    for st_name, st in (("no start", None), ("start", start)):
        name = "%s/pipeline/%s" % (tag, st_name)

        def separation(*x):
            return rp.min_time_fleet_separation(x[:3], x[3], x[4], start=x[5])[:2]
        value, _ = rec.derivatives(name + "/separation", separation, p + [lo, hi, st])
        radius = torch.sqrt(torch.where(torch.isnan(value), torch.ones_like(value), value) * 1.5)

        def contact(*x):
            return (rp.min_time_fleet_contact(x[:3], x[3], x[4], x[5], start=x[6])[0],)
        t, = rec.derivatives(name + "/contact", contact, p + [radius, lo, hi, st])
        rec.count("pipeline contacts", ~torch.isnan(t))
        rec.count("pipeline contact queries", torch.ones_like(t, dtype=torch.bool))


def bits(path, tree):
    import numpy as np
    torch, rp = load(tree)
    rec = Recorder(torch)
    n = 3
    for d in (2, 3):
        for m in (2, 3, 7):
            for k in (1, 4):
                seed = 100 * d + 10 * m + k
                tag = "d %d m %d k %d" % (d, m, k)
                fleet = make_fleet(torch, n, m, d, seed, end_velocities=(m == 3))
                lo, hi = make_windows(torch, n, k, seed + 1)
                start = (0.3 * torch.rand((n, m), dtype=torch.float64, generator=torch.Generator().manual_seed(seed + 2))).to(DEV)
                fleet_functions(rec, rp, tag, fleet, start, lo, hi, m)
                pipelines(rec, rp, tag, n, m, d, k, seed + 3, start, lo, hi)
                print("%s done: %d arrays so far" % (tag, len(rec.arrays)), flush=True)
    print("times by class: " + ", ".join("%s %d" % kv for kv in sorted(rec.classes.items())))
    np.savez(path, **rec.arrays)
    print("%d arrays, %d bytes -> %s" % (len(rec.arrays), sum(a.nbytes for a in rec.arrays.values()), path))


def compare(path_a, path_b):
    import numpy as np
    a, b = np.load(path_a), np.load(path_b)
    digest = lambda x: hashlib.sha1(np.ascontiguousarray(x).tobytes()).hexdigest()      # noqa: E731
    differing = sorted(set(a.files) ^ set(b.files))
    total = 0
    for name in sorted(set(a.files) & set(b.files)):
        x, y = a[name], b[name]
        total += x.nbytes
        if x.shape != y.shape or x.dtype != y.dtype or digest(x) != digest(y):
            differing.append(name)
    print("%d / %d arrays, %d bytes a side, %d arrays differ" % (len(a.files), len(b.files), total, len(differing)))
    for name in differing[:40]:
        print("  differs: %s" % name)
    return 1 if differing else 0


def time_one(tree):
    import numpy as np
    torch, rp = load(tree)
    n, m, k, d = 3, 7, 4, 3
    fleet = make_fleet(torch, n, m, d, 7, end_velocities=True)
    lo, hi = make_windows(torch, n, k, 8)
    start = (0.3 * torch.rand((n, m), dtype=torch.float64, generator=torch.Generator().manual_seed(9))).to(DEV)
    with torch.no_grad():
        level = rp.trajectory_fleet_separation(fleet, lo, hi)[0] * 1.5
        level = torch.where(torch.isnan(level), torch.ones_like(level), level)
    leaf = lambda t: t.detach().clone().requires_grad_(True)      # noqa: E731
    fleet, lo, hi, start, level = [leaf(t) for t in fleet], leaf(lo), leaf(hi), leaf(start), leaf(level)
    functions = (
        ("separation", lambda: rp.trajectory_fleet_separation(fleet, lo, hi)[0]),
        ("separation, start", lambda: rp.trajectory_fleet_separation(fleet, lo, hi, start=start)[0]),
        ("contact", lambda: rp.trajectory_fleet_contact(fleet, None, lo, hi, level_sq=level)),
        ("contact, start", lambda: rp.trajectory_fleet_contact(fleet, None, lo, hi, level_sq=level, start=start)),
    )
    leaves = fleet + [lo, hi, start, level]
    times = {name: [] for name, _ in functions}
    for r in range(WARMUP + REPS):
        for name, f in functions:
            torch.cuda.synchronize()
            t0 = clock.perf_counter()
            out = f()
            torch.autograd.grad(torch.nan_to_num(out).sum(), leaves, allow_unused=True)
            torch.cuda.synchronize()
            if r >= WARMUP:
                times[name].append(1e3 * (clock.perf_counter() - t0))
    print(json.dumps({name: float(np.median(t)) for name, t in times.items()}), flush=True)


def timing(parent, new):
    import numpy as np
    sides = (("parent", parent), ("new", new or ROOT))
    rounds = {side: [] for side, _ in sides}
    for r in range(ROUNDS):
        for side, tree in sides:      # alternating, a fresh process each, ended at its own time limit
            done = subprocess.run([sys.executable, os.path.abspath(__file__), "time-one", tree], capture_output=True, text=True, timeout=LIMIT)
            if done.returncode != 0:
                sys.stderr.write(done.stdout + done.stderr)
                return done.returncode or 1
            rounds[side].append(json.loads(done.stdout.strip().splitlines()[-1]))
            print("round %d %-6s %s" % (r, side, "  ".join("%s %.4f" % kv for kv in rounds[side][-1].items())), flush=True)
    print("| function | parent, ms per round | new, ms per round | parent median | new median | parent's spread | new / parent | within |")
    print("|---|---|---|---|---|---|---|---|")
    met = True
    for name in rounds["parent"][0]:
        old, fresh = [x[name] for x in rounds["parent"]], [x[name] for x in rounds["new"]]
        spread, ratio = max(old) / min(old), float(np.median(fresh)) / float(np.median(old))
        met = met and ratio <= spread
        print("| %s | %s | %s | %.4f | %.4f | %.4f | %.4f | %s |" % (name, " ".join("%.4f" % x for x in old), " ".join("%.4f" % x for x in fresh),
                                                                  float(np.median(old)), float(np.median(fresh)), spread, ratio,
                                                                  "yes" if ratio <= spread else "**no**"))
    print("host cost: " + ("met" if met else "NOT met"))
    return 0


if __name__ == "__main__":
    mode, rest = (sys.argv[1] if len(sys.argv) > 1 else ""), sys.argv[2:]
    if mode == "bits" and len(rest) in (1, 2):
        bits(rest[0], rest[1] if len(rest) == 2 else None)
    elif mode == "compare" and len(rest) == 2:
        sys.exit(compare(*rest))
    elif mode == "time" and len(rest) in (1, 2):
        sys.exit(timing(rest[0], rest[1] if len(rest) == 2 else None))
    elif mode == "time-one" and len(rest) in (0, 1):
        time_one(rest[0] if rest else None)
    else:
        sys.exit(__doc__)
