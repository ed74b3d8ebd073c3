"""The size sweep behind kOverlapMinProblems (rocket_path_amd/csrc/rp_batch.cpp) and the cost of the event hops in a restart/solve loop.

    python profiles/solve_overlap_sweep.py [--reps 5]

1. Wall clock over 40 back-to-back fused solves of 40 batches on ONE stream, at n = 65,536, 262,144 and 1,048,576, with the overlap off
   (mode 0) and with every eligible solve overlapped (mode 2), alternating on one device; the median and the range of the repetitions.
   The rule: the threshold of mode 1 is the smallest of the three sizes at which mode 2 is not slower.
2. 160 (restart, solve) pairs on a ring of 16 batches of 1,048,576 problems -- bench.py's conditioning loop -- in mode 0 and in mode 1:
   no two solves follow one another directly there, so nothing overlaps and the difference is what the bookkeeping costs.
Results go to stdout (kept as profiles/solve_overlap_ab.log)."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import numpy as np          # noqa: E402
import torch          # noqa: E402

import rocket_path_amd as rp          # noqa: E402


def burst(batches, mode):
    rp.solve_overlap(mode)
    for b in batches:
        b.restart()
    for b in batches[:8]:          # a little load right before the clock starts
        b.solve()
    for b in batches[:8]:
        b.restart()
    batches[0].sync()
    t0 = time.perf_counter()
    for b in batches:
        b.solve()
    batches[0].sync()
    return (time.perf_counter() - t0) * 1e3 / len(batches)


def pairs(ring, mode, count=160):
    rp.solve_overlap(mode)
    ring[0].sync()
    t0 = time.perf_counter()
    for j in range(count):
        b = ring[j % len(ring)]
        b.restart()
        b.solve()
    ring[0].sync()
    return (time.perf_counter() - t0) * 1e3 / count


def family(n, count, d_pos):
    lead = rp.Batch(n)
    bs = [lead] + [rp.Batch(n, stream=lead.stream()) for _ in range(count - 1)]
    for b in bs:
        b.set_problems_device(d_pos, d_pos + 8 * n, d_pos + 16 * n)
    return bs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    print("device: %s" % rp.device_id(0))
    for n in (65536, 262144, 1048576):
        pos = np.stack(rp.problems.generate(20240, 0, n, rp.problems.DIST_MONOTONE))
        d = torch.from_numpy(pos).to(torch.device("cuda", 0))          # resident before anything is timed
        torch.cuda.synchronize()
        bs = family(n, 40, d.data_ptr())
        for _ in range(2):          # untimed: code objects, clocks
            burst(bs, 0)
            burst(bs, 2)
        ms = {0: [], 2: []}
        for _ in range(args.reps):
            for mode in (0, 2):
                ms[mode].append(burst(bs, mode))
        steps = bs[0].reduce()["total_steps"]
        for mode in (0, 2):
            m = statistics.median(ms[mode])
            print("n = %8d  mode %d  ms per solve: median %.5f  min %.5f  max %.5f  (%.2f G steps/s)  runs %s"
                  % (n, mode, m, min(ms[mode]), max(ms[mode]), steps / m / 1e6, " ".join("%.5f" % x for x in ms[mode])))
        print("n = %8d  mode 0 / mode 2 = %.4f" % (n, statistics.median(ms[0]) / statistics.median(ms[2])))
        if n == 1048576:
            ring = bs[:16]
            for _ in range(2):
                pairs(ring, 0)
                pairs(ring, 1)
            pm = {0: [], 1: []}
            for _ in range(args.reps):
                for mode in (0, 1):
                    pm[mode].append(pairs(ring, mode))
            for mode in (0, 1):
                print("160 (restart, solve) pairs, n = %d, mode %d  ms per pair: median %.5f  min %.5f  max %.5f"
                      % (n, mode, statistics.median(pm[mode]), min(pm[mode]), max(pm[mode])))
        for b in bs[1:]:
            b.close()
        bs[0].close()
    rp.solve_overlap(1)
    print("counters: %s" % rp.solve_overlap_stats())


if __name__ == "__main__":
    main()
