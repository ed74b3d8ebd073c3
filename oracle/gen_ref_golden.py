#!/usr/bin/env python3
"""Generate tests/golden/ref_outputs.npz -- needs oracle/_ref (make -C oracle ref, from a reference tree).

TEST INFRASTRUCTURE ONLY.  Records what the reference's OWN functions (oracle/_ref/libref_hotpath.so) and its vendored Eigen
QR (oracle/_ref/libeigen_qr_ref.so) compute on the inputs of tests/ref_cases.py, so that tests/test_oracle_reference.py and
tests/test_oracle_golden.py pin the oracle to the reference wherever the reference is absent; where it is present the same
tests also recompute these outputs from it and require them unchanged.  Outputs the tests compare bit for bit are kept
as SHA-256 digests (tests/ref_cases.digest); values are kept only where a test compares within a tolerance: one step's
(v, t0, t1), the gated solves' (v, t0, t1), the KKT and generic solutions, Eigen's squared residual norms.

    python oracle/gen_ref_golden.py        # rewrites tests/golden/ref_outputs.npz
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ref_cases  # noqa: E402
import oracle_api  # noqa: E402
from oracle_api import Oracle, Reference  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "ref_outputs.npz")


def main():
    orc, orc_e, ref = Oracle(), Oracle(eigen=True), Reference()
    D = ref_cases.digest
    out = {"init_default_f3": ref.init_default(3), "init_default_f4": ref.init_default(4), "init_stuck": ref.init_stuck()}
    for v in (3, 4):
        out["model_f%d_sha256" % v] = D(*ref_cases.model_outputs(ref, v, ref_cases.model_states(orc, v)))
        a = ref_cases.single_step_states(orc, v)
        ref.batch_steps(v, a, 1)
        out["single_step_f%d" % v], out["single_step_f%d_sha256" % v] = a[:, :3], D(a)
        start = ref_cases.infeasible_starts(orc, v)
        nviol = ref_cases.violated_counts(orc, v, start)
        moved = ref.batch_move_toward_feasibility(v, start.copy())
        for k in range(5):
            out["feasibility_move_f%d_violated%d_sha256" % (v, k)] = D(moved[nviol == k])
    for d in (0, 1, 2):
        a = ref_cases.gated_starts(orc, d)
        it, _ = ref.batch_solve_gated(3, a, 1e-8, 200)
        out["gated_d%d" % d] = a[:, :3]
        out["gated_d%d_sha256" % d], out["gated_iters_d%d_sha256" % d] = D(a), D(np.asarray(it, dtype=np.int32))
    solved = [orc_e.ref_qr_solve(A, b, force_dynamic=True) for _, _, A, b in ref_cases.qr_systems()]
    out["qr_dynamic_sha256"] = D(np.concatenate([x for x, _ in solved]), np.array([nz for _, nz in solved], dtype=np.int32))
    # tests/test_oracle_golden.py: the oracle's own QR against Eigen's on the Newton step's and the feasibility move's systems
    kkt, generic, residuals = ref_cases.qr_cases(orc, np.load(os.path.join(ROOT, "tests", "golden", "f3_batch.npz"))["init"])
    solved = [orc_e.ref_qr_solve(M, r) for M, r in kkt]
    out["kkt_x"], out["kkt_nonzero_pivots"] = np.array([x for x, _ in solved]), np.array([nz for _, nz in solved], dtype=np.int32)
    out["generic_x"] = np.concatenate([orc_e.ref_qr_solve(A, b)[0] for A, b in generic])
    out["generic_x_dynamic"] = np.concatenate([orc_e.ref_qr_solve(A, b, force_dynamic=True)[0] for A, b in generic])
    out["residual_squared_norm"] = np.array([orc_e.ref.ref_squared_norm(11, r.ctypes.data_as(oracle_api._dp)) for _, _, r in residuals])
    solved = [orc_e.ref_qr_solve(A, e, force_dynamic=True) for _, A, e in ref_cases.gram_systems(orc)]
    out["gram_sha256"] = D(np.concatenate([x for x, _ in solved]), np.array([nz for _, nz in solved], dtype=np.int32))
    np.savez_compressed(OUT, **out)
    print("wrote %s (%d bytes)" % (OUT, os.path.getsize(OUT)))


if __name__ == "__main__":
    main()
