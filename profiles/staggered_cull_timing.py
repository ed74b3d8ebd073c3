"""Timing of the staggered fleet contact query with the broad phase in front (rp_trajectory_fleet_contact_staggered_culled; DESIGN.md
section 31) against the PARENT commit's library running rp_trajectory_fleet_contact_staggered on the same inputs.

    python profiles/staggered_cull_timing.py PARENT_LIB M D K      PARENT_LIB: librp_batch.so built from a checkout of the parent commit

One (m, d, k) per run, so that a caller can put every step under a time limit of its own; the lines are printed, and
profiles/staggered_cull_timing.log is the twelve runs' output one after the other (m = 16, 64, 256; d = 2, 3; k = 1, 8).

Conventions of profiles/fleet_cull_timing.py: HIP events on torch's current stream, 3 warm-up and 20 timed repetitions, the contenders
alternating within each repetition, inputs made on the device, n scenes with n m (m - 1) / 2 about 1,048,576 (scene, pair) problems; the
vehicles its random family with vehicle v moved by `spacing` times its grid cell; the level per scene.  The starts of a scene are
U(0, 1) times `spread` times the scene's shortest total time, as the tests'.  Rows:
    nothing removable   spread 0.5, spacing 0, radius 1000, the windows drawn inside [the last start, the first end] of the scene: every
                        pair is under way in every window and every box is within the level of every other -- what the option costs
    the family          spread 2 and spread 8, spacing 6, radius 3, the windows' ends the sorted pair of two U(0, 1) draws across the
                        scene's span [the first start, the last end]
    90 %, 99 % culled   spread 2 with the spacing found by bisection on rp_trajectory_fleet_contact_staggered_candidates' flags
Timed per repetition:
    parent              the parent library's rp_trajectory_fleet_contact_staggered
    culled              this library's rp_trajectory_fleet_contact_staggered_culled, all of it
    boxes               rp_trajectory_fleet_reach_staggered alone (no slacks, totals or speed bounds: a few stores fewer than inside the call)
    boxes+sieve+list    rp_trajectory_fleet_contact_staggered_candidates: everything but the search
The culled call's bits are compared with the parent's in all three outputs.  The figures are recorded; the one thing checked is the
issue's: wherever at least 60 % of the pairs are culled the call is faster than the parent by more than the parent's own max / min."""
import ctypes
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import rocket_path_amd as rp  # noqa: E402
from rocket_path_amd import capi  # noqa: E402

REPS, WARMUP = 20, 3
PROBLEMS = 1 << 20
NAMES = ("parent", "culled", "boxes", "boxes+sieve+list")


def timed(times, name, run):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    run()
    stop.record()
    stop.synchronize()
    times[name].append(start.elapsed_time(stop))


def main(parent_path, m, d, k):
    dev = torch.device("cuda:0")
    parent = ctypes.CDLL(os.path.abspath(parent_path))
    restype, argtypes = capi.SIGNATURES["rp_trajectory_fleet_contact_staggered"]
    parent.rp_trajectory_fleet_contact_staggered.restype, parent.rp_trajectory_fleet_contact_staggered.argtypes = restype, argtypes
    parent.rp_version.restype = ctypes.c_char_p
    assert not hasattr(parent, "rp_trajectory_fleet_contact_staggered_culled"), "PARENT_LIB is not the parent's library"
    lines = []
    if (m, d, k) == (16, 2, 1):
        lines.append("device: %s (%s); parent library: %s" % (torch.cuda.get_device_name(0), rp.device_id(0), parent.rp_version().decode()))
    gen = torch.Generator(device=dev).manual_seed(31 + 1000 * m + 10 * d + k)
    uniform = lambda shape, lo, hi: torch.rand(shape, dtype=torch.float64, device=dev, generator=gen) * (hi - lo) + lo      # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
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
    out = [torch.empty((n, pairs, k), dtype=torch.float64, device=dev) for _ in range(6)]      # parent's time, local time, rate; culled's
    kept = torch.empty((n, pairs), dtype=torch.uint8, device=dev)
    boxes = torch.empty((2, d, n * m * k + (n * m * k & 1)), dtype=torch.float64, device=dev)      # each array 16-byte aligned
    size = capi.trajectory_fleet_contact_staggered_culled_workspace(n, m, k, d)
    work = torch.empty(size, dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def scene(spread, inside):
        """(start, lo, hi): the starts, and the windows across the scene's span -- or, `inside`, across [the last start, the first end]"""
        start = (unit_start * spread * shortest).contiguous()
        ends = start + total.min(dim=2).values
        first, last = (start.max(dim=1, keepdim=True).values, ends.min(dim=1, keepdim=True).values) if inside else \
                      (start.min(dim=1, keepdim=True).values, (start + total.max(dim=2).values).max(dim=1, keepdim=True).values)
        assert bool((first < last).all())
        return start, (first + draws[:, :, 0] * (last - first)).contiguous(), (first + draws[:, :, 1] * (last - first)).contiguous()

    def tables(spacing):
        six = [(p + spacing * cell).contiguous() for p in base] + [vel1, dur0, dur1]
        flat = [[t[:, :, c].reshape(n * m).contiguous() for t in six] for c in range(d)]
        table = [a for s in flat for a in (s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr())]
        return flat, table

    def culled_share(spacing, start, lo, hi, level):
        flat, table = tables(spacing)
        capi.trajectory_fleet_contact_staggered_candidates(0, stream, n, m, k, d, table, start.data_ptr(), level.data_ptr(), 0, lo.data_ptr(),
                                                           hi.data_ptr(), work.data_ptr(), size, kept.data_ptr())
        return 1.0 - float(kept.double().mean())

    near = torch.full((n, k), 9.0, dtype=torch.float64, device=dev)
    wide = torch.full((n, k), 1000.0 ** 2, dtype=torch.float64, device=dev)
    rows = [("nothing removable", 0.0, scene(0.5, True), wide), ("the family, spread 2", 6.0, scene(2.0, False), near),
            ("the family, spread 8", 6.0, scene(8.0, False), near)]
    two = scene(2.0, False)
    for target in (0.90, 0.99):      # the culled share grows with the spacing
        low, high = 0.0, 4096.0
        for _ in range(24):
            mid = 0.5 * (low + high)
            low, high = (mid, high) if culled_share(mid, *two, near) < target else (low, mid)
        rows.append(("%d %% culled" % round(100 * target), high, two, near))
    lines.append("m = %d, d = %d, k = %d: n %d scenes x %d pairs, %d warm-up + %d timed repetitions, median (min, max) ms"
                 % (m, d, k, n, pairs, WARMUP, REPS))
    ok = True
    for what, spacing, (start, lo, hi), level in rows:
        flat, table = tables(spacing)
        share = culled_share(spacing, start, lo, hi, level)
        parent_table = capi.axes_table(table, d)
        times = {name: [] for name in NAMES}
        for _ in range(WARMUP + REPS):
            timed(times, "parent", lambda: parent.rp_trajectory_fleet_contact_staggered(0, ctypes.c_void_p(stream), n, m, k, d, parent_table, vp(start),
                                                                                         vp(level), 0, vp(lo), vp(hi), vp(out[0]), vp(out[1]), vp(out[2])))
            timed(times, "culled", lambda: capi.trajectory_fleet_contact_staggered_culled(0, stream, n, m, k, d, table, start.data_ptr(), level.data_ptr(), 0,
                                                                                          lo.data_ptr(), hi.data_ptr(), out[3].data_ptr(), out[4].data_ptr(),
                                                                                          out[5].data_ptr(), work.data_ptr(), size))
            timed(times, "boxes", lambda: capi.trajectory_fleet_reach_staggered(0, stream, n, m, k, d, table, start.data_ptr(), lo.data_ptr(), hi.data_ptr(),
                                                                                [boxes[0, c].data_ptr() for c in range(d)],
                                                                                [boxes[1, c].data_ptr() for c in range(d)]))
            timed(times, "boxes+sieve+list", lambda: capi.trajectory_fleet_contact_staggered_candidates(0, stream, n, m, k, d, table, start.data_ptr(),
                                                                                                        level.data_ptr(), 0, lo.data_ptr(), hi.data_ptr(),
                                                                                                        work.data_ptr(), size, kept.data_ptr()))
        times = {name: t[WARMUP:] for name, t in times.items()}
        same = all(bool(torch.equal(out[i].view(torch.int64), out[i + 3].view(torch.int64))) for i in range(3))
        med = {name: float(np.median(times[name])) for name in NAMES}
        ratio, own = med["culled"] / med["parent"], max(times["parent"]) / min(times["parent"])
        lines.append("  %s (spacing %.3f, radius %.1f): %5.1f %% of the pairs culled, %4.1f %% of the queries with a contact; bits %s the parent's"
                     % (what, spacing, float(level[0, 0]) ** 0.5, 100 * share, 100 * float(torch.isfinite(out[0]).double().mean()),
                        "equal" if same else "DIFFER FROM"))
        for name in NAMES:
            t = times[name]
            lines.append("    %-18s %9.4f (%9.4f, %9.4f) ms" % (name, np.median(t), min(t), max(t)))
        lines.append("    culled / parent %.3f (parent's own max / min %.3f); boxes %.4f, sieve + list %.4f, search %.4f ms"
                     % (ratio, own, med["boxes"], med["boxes+sieve+list"] - med["boxes"], med["culled"] - med["boxes+sieve+list"]))
        if share >= 0.60 and not ratio * own < 1.0:
            lines.append("    NOT faster than the parent by more than its own spread, at %.1f %% culled" % (100 * share))
            ok = False
        ok = ok and same
        del flat
    sys.stdout.write("\n".join(lines) + "\n")
    sys.stdout.flush()
    return 0 if ok else 1


if __name__ == "__main__":
    if len(sys.argv) != 5:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], *[int(a) for a in sys.argv[2:]]))
