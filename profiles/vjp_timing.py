"""Backward (rp_batch_solution_vjp) against forward (set_problems_device + fused gated solve) timing, HIP events on the batch
stream, at 65,536 and 1,048,576 of bench.py's problems.  Prints one line per size; run on an MI355X:
    python profiles/vjp_timing.py > profiles/vjp_timing.log"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import rocket_path_amd as rp  # noqa: E402

REPS, WARMUP = 20, 3


def main():
    print("device: %s (%s)" % (torch.cuda.get_device_name(0), rp.device_id(0)))
    for n in (65536, 1 << 20):
        p = [torch.as_tensor(x, device="cuda:0") for x in rp.problems.generate(12345, 0, n, rp.problems.DIST_MONOTONE)]
        g = [torch.randn(n, dtype=torch.float64, device="cuda:0") for _ in range(3)]
        bars = [torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(3)]
        torch.cuda.synchronize()
        fwd, bwd = [], []
        with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            for r in range(WARMUP + REPS):
                b.event_record(0)
                b.set_problems_device(*[x.data_ptr() for x in p])
                b.solve(1e-8, 200, 0)
                b.event_record(1)
                b.solution_vjp(*[x.data_ptr() for x in g], *[x.data_ptr() for x in bars])
                b.event_record(2)
                b.sync()
                if r >= WARMUP:
                    fwd.append(b.event_elapsed_ms(0, 1))
                    bwd.append(b.event_elapsed_ms(1, 2))
        f, k = np.median(fwd), np.median(bwd)
        bytes_moved = n * (16 * 8 + 3 * 8 + 3 * 8 + 4)      # state + gathered gradients + scattered results + prob_of
        print("n %8d  forward %.4f ms  backward %.4f ms (min %.4f, max %.4f)  backward/forward %.3f  backward %.2f TB/s of %d B/problem"
              % (n, f, k, min(bwd), max(bwd), k / f, bytes_moved / (k * 1e-3) / 1e12, bytes_moved // n))


if __name__ == "__main__":
    main()
