"""Timing of the fleet contact query with the broad phase in front (rp_trajectory_fleet_contact_culled) against the
PARENT commit's library running rp_trajectory_fleet_contact on the same inputs.

    python profiles/fleet_cull_timing.py PARENT_LIB      PARENT_LIB: librp_batch.so built from a checkout of the parent commit

Conventions of profiles/fleet_timing.py: HIP events on torch's current stream, 3 warm-up and 20 timed repetitions, the contenders
alternating within each repetition, inputs made on the device, n scenes with n m (m - 1) / 2 about 1,048,576 (scene, pair) problems.
m = 16, 64, 256 vehicles per scene, d = 2, 3 axes, k = 1, 8 queries.  The vehicles are the tests' random family (positions U(-5, 5),
velocities U(-20, 20), durations U(0.05, 2); rest-to-rest tables) with vehicle v moved by `spacing` times its grid cell (side =
ceil(m ** (1 / d)), coordinate (v // side ** c) % side on axis c); the windows' ends the sorted pair of two U(0, 1) draws across each
scene's domain (no window before t = 0: such a window keeps its scene's pairs, and with k = 8 the culled share could not reach 99 %);
the level per scene, 3.0 ** 2.  Per (m, d, k): spacing 0 with the radius 1000 -- every box is within the level of every other, nothing
can be culled, and no pair ever reaches the level from outside, so every query walks all its pieces: what the option costs --; spacing 0
with the radius 3, the family as it comes; and the spacings found by bisection on rp_trajectory_fleet_contact_candidates' flags at which
about 50 %, 90 % and 99 % of the pairs are culled (a share the family already has at spacing 0 is left out); the share is logged with
every row.  Timed per repetition:
    parent              the parent library's rp_trajectory_fleet_contact
    culled              this library's rp_trajectory_fleet_contact_culled, all of it
    boxes               rp_trajectory_fleet_reach alone (it writes no slacks: a few stores fewer than the pass inside the culled call)
    boxes+sieve+list    rp_trajectory_fleet_contact_candidates: everything but the search
from which sieve + list = candidates - boxes and search = culled - candidates (medians).  The public entries do not separate the sieve
from the list's three kernels.  The culled call's bits are compared with the parent's.  No threshold: the figures are recorded, not
asserted.  Writes profiles/fleet_cull_timing.log beside this script (and prints the same lines); run on an MI355X."""
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
TARGETS = (0.50, 0.90, 0.99)
NAMES = ("parent", "culled", "boxes", "boxes+sieve+list")


def timed(times, name, run):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    run()
    stop.record()
    stop.synchronize()
    times[name].append(start.elapsed_time(stop))


def main(parent_path):
    dev = torch.device("cuda:0")
    parent = ctypes.CDLL(os.path.abspath(parent_path))
    restype, argtypes = capi.SIGNATURES["rp_trajectory_fleet_contact"]
    parent.rp_trajectory_fleet_contact.restype, parent.rp_trajectory_fleet_contact.argtypes = restype, argtypes
    parent.rp_version.restype = ctypes.c_char_p
    assert not hasattr(parent, "rp_trajectory_fleet_contact_culled"), "PARENT_LIB is not the parent's library"
    lines = ["device: %s (%s); parent library: %s" % (torch.cuda.get_device_name(0), rp.device_id(0), parent.rp_version().decode())]
    gen = torch.Generator(device=dev).manual_seed(30)
    uniform = lambda shape, lo, hi: torch.rand(shape, dtype=torch.float64, device=dev, generator=gen) * (hi - lo) + lo      # noqa: E731
    vp = lambda t: ctypes.c_void_p(t.data_ptr())      # noqa: E731
    for m in (16, 64, 256):
        pairs = m * (m - 1) // 2
        n = max(1, round(PROBLEMS / pairs))
        for d in (2, 3):
            side = 1
            while side ** d < m:
                side += 1
            v = torch.arange(m, device=dev)
            cell = torch.stack([(v // side ** c) % side for c in range(d)], dim=1).to(torch.float64)      # (m, d)
            base = [uniform((n, m, d), -5.0, 5.0) for _ in range(3)]
            vel1, dur0, dur1 = uniform((n, m, d), -20.0, 20.0), uniform((n, m, d), 0.05, 2.0), uniform((n, m, d), 0.05, 2.0)
            end = (dur0 + dur1).reshape(n, m * d).min(dim=1, keepdim=True).values
            for k in (1, 8):
                draws = torch.sort(uniform((n, k, 2), 0.0, 1.0), dim=2).values
                lo, hi = (draws[:, :, 0] * end).contiguous(), (draws[:, :, 1] * end).contiguous()
                level = torch.full((n, k), 9.0, dtype=torch.float64, device=dev)
                wide = torch.full((n, k), 1000.0 ** 2, dtype=torch.float64, device=dev)
                out = [torch.empty((n, pairs, k), dtype=torch.float64, device=dev) for _ in range(4)]      # parent's time, rate; culled's
                kept = torch.empty((n, pairs), dtype=torch.uint8, device=dev)
                boxes = torch.empty((2, d, n * m * k + (n * m * k & 1)), dtype=torch.float64, device=dev)      # each array 16-byte aligned
                size = capi.trajectory_fleet_contact_culled_workspace(n, m, k, d)
                work = torch.empty(size, dtype=torch.uint8, device=dev)
                stream = torch.cuda.current_stream(dev).cuda_stream

                def tables(spacing):
                    six = [(p + spacing * cell).contiguous() for p in base] + [vel1, dur0, dur1]
                    flat = [[t[:, :, c].reshape(n * m).contiguous() for t in six] for c in range(d)]
                    table = [a for s in flat for a in (s[0].data_ptr(), s[1].data_ptr(), s[2].data_ptr(), 0, 0, s[3].data_ptr(), s[4].data_ptr(), s[5].data_ptr())]
                    return flat, table

                def culled_share(spacing, level=level):
                    flat, table = tables(spacing)
                    capi.trajectory_fleet_contact_candidates(0, stream, n, m, k, d, table, level.data_ptr(), 0, lo.data_ptr(), hi.data_ptr(),
                                                             work.data_ptr(), size, kept.data_ptr())
                    return 1.0 - float(kept.double().mean())

                rows = [(0.0, wide), (0.0, level)]      # nothing can be culled; the family as it comes
                at_rest = culled_share(0.0)
                for target in TARGETS:      # the culled share grows with the spacing
                    if at_rest >= target:
                        continue
                    low, high = 0.0, 4096.0
                    for _ in range(24):
                        mid = 0.5 * (low + high)
                        low, high = (mid, high) if culled_share(mid) < target else (low, mid)
                    rows.append((high, level))
                lines.append("m = %d, d = %d, k = %d: n %d scenes x %d pairs, %d warm-up + %d timed repetitions, median (min, max) ms"
                             % (m, d, k, n, pairs, WARMUP, REPS))
                for row, (spacing, level) in enumerate(rows):
                    flat, table = tables(spacing)
                    share = culled_share(spacing, level)
                    parent_table = capi.axes_table(table, d)
                    times = {name: [] for name in NAMES}
                    for _ in range(WARMUP + REPS):
                        timed(times, "parent", lambda: parent.rp_trajectory_fleet_contact(0, ctypes.c_void_p(stream), n, m, k, d, parent_table, vp(level), 0,
                                                                                         vp(lo), vp(hi), vp(out[0]), vp(out[1])))
                        timed(times, "culled", lambda: capi.trajectory_fleet_contact_culled(0, stream, n, m, k, d, table, level.data_ptr(), 0, lo.data_ptr(),
                                                                                            hi.data_ptr(), out[2].data_ptr(), out[3].data_ptr(),
                                                                                            work.data_ptr(), size))
                        timed(times, "boxes", lambda: capi.trajectory_fleet_reach(0, stream, n, m, k, d, table, lo.data_ptr(), hi.data_ptr(),
                                                                                  [boxes[0, c].data_ptr() for c in range(d)],
                                                                                  [boxes[1, c].data_ptr() for c in range(d)]))
                        timed(times, "boxes+sieve+list", lambda: capi.trajectory_fleet_contact_candidates(0, stream, n, m, k, d, table, level.data_ptr(), 0,
                                                                                                          lo.data_ptr(), hi.data_ptr(), work.data_ptr(), size,
                                                                                                          kept.data_ptr()))
                    times = {name: t[WARMUP:] for name, t in times.items()}
                    same = all(bool(torch.equal(x.view(torch.int64), y.view(torch.int64))) for x, y in ((out[0], out[2]), (out[1], out[3])))
                    med = {name: float(np.median(times[name])) for name in NAMES}
                    lines.append("  spacing %9.3f, radius %6.1f: %5.1f %% of the pairs culled, %4.1f %% of the queries with a contact; bits %s the parent's"
                                 % (spacing, float(level[0, 0]) ** 0.5, 100 * share, 100 * float(torch.isfinite(out[0]).double().mean()), "equal" if same else "DIFFER FROM"))
                    for name in NAMES:
                        t = times[name]
                        lines.append("    %-18s %9.4f (%9.4f, %9.4f) ms" % (name, np.median(t), min(t), max(t)))
                    lines.append("    culled / parent %.3f (parent's own max / min %.3f); boxes %.4f, sieve + list %.4f, search %.4f ms"
                                 % (med["culled"] / med["parent"], max(times["parent"]) / min(times["parent"]), med["boxes"],
                                    med["boxes+sieve+list"] - med["boxes"], med["culled"] - med["boxes+sieve+list"]))
                    del flat
                    sys.stdout.write("\n".join(lines[-7 if row == 0 else -6:]) + "\n")
                    sys.stdout.flush()
    text = "\n".join(lines) + "\n"
    with open(os.path.join(HERE, "fleet_cull_timing.log"), "w") as f:
        f.write(text)


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
