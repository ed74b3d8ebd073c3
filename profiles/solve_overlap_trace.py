"""Do consecutive k_solve_chunks launches of bench.py's timed region overlap?  Reads the kernel trace of

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python bench.py --gpus 1 --no-extras --no-cpu-baseline

(no counters in that run) and prints start and end of every launch of the timed region, relative to the region's first start.

    python profiles/solve_overlap_trace.py DIR [--conditioning 160] [--warmup 3] [--steps 20]

The gated kernel's launches come in bench.py's order: the conditioning solves, the warmup passes, then the K timed ones."""
import argparse
import csv
import glob
import os


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("dir")
    ap.add_argument("--conditioning", type=int, default=160)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=20)
    args = ap.parse_args()
    files = sorted(glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True))
    if not files:
        raise SystemExit("no *kernel_trace.csv under %s" % args.dir)
    rows = []
    for f in files:
        for r in csv.DictReader(open(f)):
            if "k_solve_chunks" in r.get("Kernel_Name", ""):
                rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r.get("Queue_Id", "?"), r.get("Stream_Id", "?")))
    rows.sort()
    first = args.conditioning + args.warmup
    region = rows[first:first + args.steps]
    if len(region) < args.steps:
        raise SystemExit("only %d k_solve_chunks launches in the trace" % len(rows))
    t0 = region[0][0]
    print("k_solve_chunks launches %d..%d of %d in the trace (the timed region); times in us from the region's first start" % (first, first + args.steps - 1, len(rows)))
    print("%4s %10s %10s %10s %8s %8s %s" % ("#", "start", "end", "duration", "queue", "stream", "overlap with the next launch"))
    overlaps = 0
    for i, (s, e, q, st) in enumerate(region):
        nxt = region[i + 1][0] if i + 1 < len(region) else None
        ov = (e - nxt) / 1e3 if nxt is not None else None
        overlaps += 1 if ov is not None and ov > 0 else 0
        print("%4d %10.1f %10.1f %10.1f %8s %8s %s" % (i, (s - t0) / 1e3, (e - t0) / 1e3, (e - s) / 1e3, q, st, "" if ov is None else "%+.1f" % ov))
    span = (max(e for _, e, _, _ in region) - t0) / 1e3
    total = sum(e - s for s, e, _, _ in region) / 1e3
    print("consecutive launches that overlap: %d of %d;  region %.1f us for %.1f us of kernel durations (%.3f)" % (overlaps, len(region) - 1, span, total, total / span))


if __name__ == "__main__":
    main()
