"""Second-derivative (rp_batch_solution_hessian) timing against the Jacobian (rp_batch_solution_jacobian), the backward
(rp_batch_solution_vjp) and the forward solve (set_problems_device + fused gated solve), HIP events on the batch stream, at 65,536
and 1,048,576 of bench.py's problems.  Prints one line per size; run on an MI355X:
    python profiles/hessian_timing.py > profiles/hessian_timing.log"""
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
        outs = [torch.empty(n, dtype=torch.float64, device="cuda:0") for _ in range(3)]
        jac = torch.empty((n, 9), dtype=torch.float64, device="cuda:0")
        hess = torch.empty((n, 27), dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()
        times = {"forward": [], "hessian": [], "hessian_nojac": [], "jacobian": [], "vjp": []}
        with rp.Batch(n, rp.VARIANT_F3, rp.DTYPE_F64, device=0) as b:
            for r in range(WARMUP + REPS):
                b.event_record(0)
                b.set_problems_device(*[x.data_ptr() for x in p])
                b.solve(1e-8, 200, 0)
                b.event_record(1)
                b.solution_hessian(jac.data_ptr(), hess.data_ptr())
                b.event_record(2)
                b.solution_hessian(0, hess.data_ptr())
                b.event_record(3)
                b.solution_jacobian(jac.data_ptr())
                b.event_record(4)
                b.solution_vjp(*[x.data_ptr() for x in g], *[x.data_ptr() for x in outs])
                b.event_record(5)
                b.sync()
                if r >= WARMUP:
                    for k, name in enumerate(times):
                        times[name].append(b.event_elapsed_ms(k, k + 1))
        med = {k: np.median(v) for k, v in times.items()}
        # bytes per problem: state + scattered results + prob_of
        moved = {"hessian": 16 * 8 + 27 * 8 + 9 * 8 + 4, "hessian_nojac": 16 * 8 + 27 * 8 + 4, "jacobian": 16 * 8 + 9 * 8 + 4,
                 "vjp": 16 * 8 + 3 * 8 + 3 * 8 + 4}
        print("n %8d  forward %.4f ms" % (n, med["forward"]) + "".join(
            "  %s %.4f ms (min %.4f, max %.4f, /forward %.3f, %.2f TB/s of %d B)"
            % (k, med[k], min(times[k]), max(times[k]), med[k] / med["forward"], moved[k] * n / (med[k] * 1e-3) / 1e12, moved[k])
            for k in ("hessian", "hessian_nojac", "jacobian", "vjp")))


if __name__ == "__main__":
    main()
