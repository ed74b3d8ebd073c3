"""A/B of the fleet contact query's broad phase (the eight rp_trajectory_fleet_reach*, *_culled*, *_candidates entries; DESIGN.md sections
30 to 32) between two builds of librp_batch.so of the same C ABI: the same bits in everything the entries write, and the same speed.
Modes, each a fresh process:

    python profiles/cull_refactor_ab.py classes                  the classes of the bits mode's pairs by the tests' NumPy models; no device
    python profiles/cull_refactor_ab.py bits OUT.npz [LIB]        everything the entries write into one file (LIB: default this tree's)
    python profiles/cull_refactor_ab.py compare A.npz B.npz       per-array SHA-1 of two such files; exit status 1 unless all are equal
    python profiles/cull_refactor_ab.py time PARENT_LIB ENTRY D K [NEW_LIB]    ENTRY: culled or staggered; one (entry, d, k) per run,
                                                                  m = 64; exit status 3 where the condition below is not met

bits: d = 1, 2, 3, n = 3 scenes of m = 2, 3, 7 vehicles, k = 1, 4; the level per scene and per pair; both window ends, lo null, hi null.
The inputs are the tests' makers': tests/staggered_cull_inputs.py's family (spacing 6 and, so that pairs are kept, spacing 0; starts
spread over 2 (k = 1) or 8 (k = 4) of the scene's shortest total time), and for the entries on one clock the same fleet with the windows
of tests/fleet_cull_gpu_cases.py's spread_inputs.  On top of them vehicle 0 of scene 1 gets a NaN duration and the last vehicle of scene
2 a start that is not finite (inf for k = 1, NaN for k = 4).  Kept: time, time_local and rate of both culled entries, d_kept, d_count
and d_list[:count]; both candidates entries' flags; both reach entries' boxes.  The pairs are counted by class -- culled and kept by
the flags; with starts also culled with every query refused (staggered_cull_inputs.refused in float64), kept with a start that is not
finite, and with a vehicle of a bad duration -- and the run fails if a class is empty.  `classes` counts the same from the models alone
(culled: every query refused or far in longdouble), so that the seeds can be chosen without a device.

time: profiles/staggered_cull_timing.py's conventions and inputs (fleet_cull_timing.py's for the entry on one clock): HIP events on
torch's current stream, 3 warm-up and 20 timed repetitions, the two libraries alternating within each repetition, about 1,048,576
(scene, pair) problems.  Two rows -- nothing removable, where the search carries the time, and 90 % culled (the spacing by bisection on
the candidates entry's flags), where boxes and sieve do --, three items per row: the culled call, the reach entry, the candidates
entry.  Per item: the new median must not be above the parent's by more than the parent's own slowest repetition over its fastest."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
N = 3
WINDOWS = ("lo hi", "no lo", "no hi")
REPS, WARMUP, PROBLEMS = 20, 3, 1 << 20


def cases():
    """(tag, fleet, start, (lo, hi) on one clock, (lo, hi) with starts, {layout: level}) of the bits mode, in numpy"""
    import separation_ref as sr
    import staggered_cull_inputs as sci
    for d in (1, 2, 3):
        for m in (2, 3, 7):
            for k in (1, 4):
                for spacing in (6.0, 0.0):
                    fleet, start, lo, hi, levels = sci.family(N, m, d, k, 2.0 if k == 1 else 8.0, spacing)
                    every = [[axis[f][:, v] for f in range(8)] for axis in fleet for v in range(m)]
                    one_clock = sr.windows(every, every, np.zeros((N, k)), 900 + k)      # fleet_cull_gpu_cases.spread_inputs'
                    fleet[0][6][1, 0] = np.nan
                    start[2, m - 1] = np.inf if k == 1 else np.nan
                    yield "d %d m %d k %d spacing %g" % (d, m, k, spacing), fleet, start, one_clock, (lo, hi), levels


def windows_of(lo, hi):
    return zip(WINDOWS, (lo, None, lo), (hi, hi, None))


class Classes:
    NAMES = ("one clock: culled", "one clock: kept", "starts: culled", "starts: kept", "starts: culled, every query refused",
             "starts: kept, a start not finite", "starts: a vehicle with a bad duration")

    def __init__(self):
        self.count = dict.fromkeys(self.NAMES, 0)

    def one_clock(self, kept):
        self.count["one clock: culled"] += int((~kept).sum())
        self.count["one clock: kept"] += int(kept.sum())

    def starts(self, kept, fleet, start, level, lo, hi):
        import staggered_cull_inputs as sci
        first, second = sci.pairs_of(start.shape[1])
        refused = sci.refused(fleet, start, level, lo, hi, T=np.float64).all(axis=2)
        loose = ~np.isfinite(start)
        bad = ~np.all([np.isfinite(axis[f]) & (axis[f] > 0) for axis in fleet for f in (6, 7)], axis=0)      # (n, m)
        self.count["starts: culled"] += int((~kept).sum())
        self.count["starts: kept"] += int(kept.sum())
        self.count["starts: culled, every query refused"] += int((~kept & refused).sum())
        self.count["starts: kept, a start not finite"] += int((kept & (loose[:, first] | loose[:, second])).sum())
        self.count["starts: a vehicle with a bad duration"] += int((bad[:, first] | bad[:, second]).sum())

    def report(self):
        print("pairs by class: " + "; ".join("%s %d" % (name, self.count[name]) for name in self.NAMES))
        empty = [name for name in self.NAMES if self.count[name] == 0]
        if empty:
            print("EMPTY: " + "; ".join(empty))
        return 1 if empty else 0


def classes():
    import staggered_cull_inputs as sci
    seen = Classes()
    for tag, fleet, start, (lo_u, hi_u), (lo_s, hi_s), levels in cases():
        first, second = sci.pairs_of(start.shape[1])
        loose = ~np.isfinite(start)
        for level in levels.values():
            for _, lo, hi in windows_of(lo_u, hi_u):
                seen.one_clock(~sci.far(fleet, np.zeros_like(start), level, lo, hi).all(axis=2))
            for _, lo, hi in windows_of(lo_s, hi_s):
                with np.errstate(all="ignore"):
                    out = sci.refused(fleet, start, level, lo, hi, T=np.float64) | sci.far(fleet, start, level, lo, hi)
                seen.starts(~out.all(axis=2) | loose[:, first] | loose[:, second], fleet, start, level, lo, hi)
    return seen.report()


def bits(path, lib_path):
    import torch
    torch.cuda.init()
    from rocket_path_amd import capi
    lib = capi.load_library(os.path.abspath(lib_path) if lib_path else capi.LIB_PATH)
    print("library: %s" % lib.rp_version().decode())
    dev = torch.device("cuda:0")
    arrays, seen = {}, Classes()
    on = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev) if x is not None else None      # noqa: E731
    ptr = lambda t: t.data_ptr() if t is not None else None      # noqa: E731

    def call(name, *args):
        status = getattr(lib, name)(0, None, *args)
        assert status == 0, (name, status, (lib.rp_last_error() or b"").decode())

    def size_of(name, *args):
        size = capi.ctypes.c_size_t(0)
        assert getattr(lib, name)(*args, capi.ctypes.byref(size)) == 0, name
        return size.value

    def keep(name, t):
        arrays[name] = t.cpu().numpy()

    for tag, fleet, start, one_clock, with_starts, levels in cases():
        n, m = start.shape
        d, pairs = len(fleet), m * (m - 1) // 2
        k = one_clock[0].shape[1]
        held = [[on(x) for x in axis] for axis in fleet]
        table = capi.axes_table([t.data_ptr() for axis in held for t in axis], d)
        t_start = on(start)
        for clock, (lo_np, hi_np), begin, stem in (("one clock", one_clock, (), "rp_trajectory_fleet_contact_"),
                                                   ("starts", with_starts, (ptr(t_start),), "rp_trajectory_fleet_contact_staggered_")):
            size = size_of(stem + "culled_workspace", n, m, k, d)
            for w_name, lo, hi in windows_of(lo_np, hi_np):
                t_lo, t_hi = on(lo), on(hi)
                name = "%s | %s | %s" % (tag, clock, w_name)
                box = torch.full((2, d, n * m * k + (n * m * k & 1)), 7.0, dtype=torch.float64, device=dev)      # each array 16-byte aligned
                call("rp_trajectory_fleet_reach" + ("_staggered" if begin else ""), n, m, k, d, table, *begin, ptr(t_lo), ptr(t_hi),
                     capi._axis_outputs([box[0, c].data_ptr() for c in range(d)], d, "d_min"),
                     capi._axis_outputs([box[1, c].data_ptr() for c in range(d)], d, "d_max"))
                keep(name + " | boxes", box)
                for layout, level in levels.items():
                    t_level = on(level)
                    outs = [torch.full((n, pairs, k), 7.0, dtype=torch.float64, device=dev) for _ in range(3 if begin else 2)]
                    work = torch.full((size,), 0x5A, dtype=torch.uint8, device=dev)
                    kept, flags = (torch.full((n, pairs), 9, dtype=torch.uint8, device=dev) for _ in range(2))
                    listed = torch.full((n * pairs,), -1, dtype=torch.int32, device=dev)
                    count = torch.full((1,), -1, dtype=torch.int32, device=dev)
                    query = (ptr(t_level), int(level.ndim == 3), ptr(t_lo), ptr(t_hi))
                    call(stem + "culled", n, m, k, d, table, *begin, *query, *[o.data_ptr() for o in outs], work.data_ptr(), size,
                         kept.data_ptr(), listed.data_ptr(), count.data_ptr())
                    call(stem + "candidates", n, m, k, d, table, *begin, *query, work.data_ptr(), size, flags.data_ptr())
                    torch.cuda.synchronize()
                    for what, o in zip(("time", "time_local", "rate") if begin else ("time", "rate"), outs):
                        keep("%s | %s | %s" % (name, layout, what), o)
                    keep("%s | %s | kept" % (name, layout), kept)
                    keep("%s | %s | count" % (name, layout), count)
                    keep("%s | %s | list" % (name, layout), listed[:int(count[0])])
                    keep("%s | %s | candidates" % (name, layout), flags)
                    if begin:
                        seen.starts(kept.cpu().numpy() != 0, fleet, start, level, lo, hi)
                    else:
                        seen.one_clock(kept.cpu().numpy() != 0)
    np.savez(path, **arrays)
    print("%d arrays, %d bytes -> %s" % (len(arrays), sum(a.nbytes for a in arrays.values()), path))
    return seen.report()


def compare(path_a, path_b):
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


def timing(parent_path, entry, d, k, new_path=None, m=64):
    import torch
    torch.cuda.init()
    from rocket_path_amd import capi
    staggered = {"culled": False, "staggered": True}[entry]
    sides = (("parent", capi.load_library(os.path.abspath(parent_path))),
             ("new", capi.load_library(os.path.abspath(new_path) if new_path else capi.LIB_PATH)))
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed((31 if staggered else 30) + 1000 * m + 10 * d + k)
    uniform = lambda shape, lo, hi: torch.rand(shape, dtype=torch.float64, device=dev, generator=gen) * (hi - lo) + lo      # noqa: E731
    pairs = m * (m - 1) // 2
    n = max(1, round(PROBLEMS / pairs))
    side = 1
    while side ** d < m:
        side += 1
    v = torch.arange(m, device=dev)
    cell = torch.stack([(v // side ** c) % side for c in range(d)], dim=1).to(torch.float64)      # (m, d)
    base = [uniform((n, m, d), -5.0, 5.0) for _ in range(3)]
    vel1, dur0, dur1 = uniform((n, m, d), -20.0, 20.0), uniform((n, m, d), 0.05, 2.0), uniform((n, m, d), 0.05, 2.0)
    total = dur0 + dur1
    shortest = total.reshape(n, m * d).min(dim=1, keepdim=True).values      # (n, 1)
    unit_start = uniform((n, m), 0.0, 1.0)
    draws = torch.sort(uniform((n, k, 2), 0.0, 1.0), dim=2).values
    outs = [torch.empty((n, pairs, k), dtype=torch.float64, device=dev) for _ in range(3 if staggered else 2)]
    kept = torch.empty((n, pairs), dtype=torch.uint8, device=dev)
    boxes = torch.empty((2, d, n * m * k + (n * m * k & 1)), dtype=torch.float64, device=dev)      # each array 16-byte aligned
    stem = "rp_trajectory_fleet_contact_staggered_" if staggered else "rp_trajectory_fleet_contact_"
    size = capi.ctypes.c_size_t(0)
    assert getattr(sides[1][1], stem + "culled_workspace")(n, m, k, d, capi.ctypes.byref(size)) == 0
    size = size.value
    work = torch.empty(size, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def scene(spread, inside):
        """(start, lo, hi) with starts: the windows across the scene's span -- or, `inside`, across [the last start, the first end]; on
        one clock (no start, lo, hi): across the scene's domain"""
        if not staggered:
            return None, (draws[:, :, 0] * shortest).contiguous(), (draws[:, :, 1] * shortest).contiguous()
        start = (unit_start * spread * shortest).contiguous()
        ends = start + total.min(dim=2).values
        first, last = (start.max(dim=1, keepdim=True).values, ends.min(dim=1, keepdim=True).values) if inside else \
                      (start.min(dim=1, keepdim=True).values, (start + total.max(dim=2).values).max(dim=1, keepdim=True).values)
        assert bool((first < last).all())
        return start, (first + draws[:, :, 0] * (last - first)).contiguous(), (first + draws[:, :, 1] * (last - first)).contiguous()

    def tables(spacing):
        six = [(p + spacing * cell).contiguous() for p in base] + [vel1, dur0, dur1]
        flat = [[t[:, :, c].reshape(n * m).contiguous() for t in six] for c in range(d)]
        table = [a for s in flat
                 for a in (s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr())]
        return flat, capi.axes_table(table, d)

    def items(lib, table, start, lo, hi, level):
        """the three timed calls of one library on one row"""
        begin = (start.data_ptr(),) if staggered else ()
        head = (0, stream, n, m, k, d, table) + begin
        query = (level.data_ptr(), 0, lo.data_ptr(), hi.data_ptr())
        box_min = capi._axis_outputs([boxes[0, c].data_ptr() for c in range(d)], d, "d_min")
        box_max = capi._axis_outputs([boxes[1, c].data_ptr() for c in range(d)], d, "d_max")
        return (("culled", lambda: getattr(lib, stem + "culled")(*head, *query, *[o.data_ptr() for o in outs], work.data_ptr(), size, None, None,
                                                                  None)),
                ("reach", lambda: getattr(lib, "rp_trajectory_fleet_reach" + ("_staggered" if staggered else ""))(*head, lo.data_ptr(), hi.data_ptr(),
                                                                                                                  box_min, box_max)),
                ("candidates", lambda: getattr(lib, stem + "candidates")(*head, *query, work.data_ptr(), size, kept.data_ptr())))

    def culled_share(spacing, start, lo, hi, level):
        flat, table = tables(spacing)
        assert items(sides[1][1], table, start, lo, hi, level)[2][1]() == 0
        return 1.0 - float(kept.double().mean())

    near = torch.full((n, k), 9.0, dtype=torch.float64, device=dev)
    wide = torch.full((n, k), 1000.0 ** 2, dtype=torch.float64, device=dev)
    two = scene(2.0, False)
    low, high = 0.0, 4096.0
    for _ in range(24):      # the culled share grows with the spacing
        mid = 0.5 * (low + high)
        low, high = (mid, high) if culled_share(mid, *two, near) < 0.90 else (low, mid)
    print("%s, m = %d, d = %d, k = %d: n %d scenes x %d pairs, %d warm-up + %d timed repetitions; parent %s, new %s"
          % (stem + "culled", m, d, k, n, pairs, WARMUP, REPS, sides[0][1].rp_version().decode(), sides[1][1].rp_version().decode()))
    print("| row | item | parent median (min, max) ms | new median (min, max) ms | new / parent | parent's max / min | within |")
    print("|---|---|---|---|---|---|---|")
    met = True
    for what, spacing, (start, lo, hi), level in (("nothing removable", 0.0, scene(0.5, True), wide), ("90 % culled", high, two, near)):
        flat, table = tables(spacing)
        share = culled_share(spacing, start, lo, hi, level)
        runs = {name: items(lib, table, start, lo, hi, level) for name, lib in sides}
        times = {(name, item): [] for name, _ in sides for item, _ in runs[name]}
        for _ in range(WARMUP + REPS):
            for j in range(3):
                for name, _ in sides:      # the two libraries alternate
                    item, run = runs[name][j]
                    begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    begin.record()
                    status = run()
                    end.record()
                    end.synchronize()
                    assert status == 0, (name, item, status)
                    times[(name, item)].append(begin.elapsed_time(end))
        for item, _ in runs["new"]:
            old, new = times[("parent", item)][WARMUP:], times[("new", item)][WARMUP:]
            ratio, own = float(np.median(new)) / float(np.median(old)), max(old) / min(old)
            met = met and ratio <= own
            print("| %s, %.1f %% culled (spacing %.3f) | %s | %.4f (%.4f, %.4f) | %.4f (%.4f, %.4f) | %.4f | %.4f | %s |"
                  % (what, 100 * share, spacing, item, np.median(old), min(old), max(old), np.median(new), min(new), max(new), ratio, own,
                     "yes" if ratio <= own else "**no**"), flush=True)
        del flat
    print("speed: " + ("met" if met else "NOT met"))
    return 0 if met else 3      # (not 1: an exception's status)


if __name__ == "__main__":
    mode, rest = (sys.argv[1] if len(sys.argv) > 1 else ""), sys.argv[2:]
    if mode == "classes" and not rest:
        sys.exit(classes())
    elif mode == "bits" and len(rest) in (1, 2):
        sys.exit(bits(rest[0], rest[1] if len(rest) == 2 else None))
    elif mode == "compare" and len(rest) == 2:
        sys.exit(compare(*rest))
    elif mode == "time" and len(rest) in (4, 5) and rest[1] in ("culled", "staggered"):
        sys.exit(timing(rest[0], rest[1], int(rest[2]), int(rest[3]), *rest[4:]))
    else:
        sys.exit(__doc__)
