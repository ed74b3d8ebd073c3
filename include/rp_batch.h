/*
 * rp_batch.h -- C ABI of the MI355X-native batched interior-point path.
 *
 * This is the one boundary between host code (the C++ `Problem` plug-in that drops into
 * rocket_path.cpp, or the Python mirror used by tests/bench) and the HIP kernels.  Plain
 * pointers and sizes only; no C++ or torch types cross it.  The library never throws:
 * every entry point returns an rp_status, and rp_last_error() has the text.
 *
 * A batch is N independent problems of one variant:
 *   RP_VARIANT_F3  two-segment cubic, 3 variables + 8 multipliers, c_i = -/+a - L
 *                  (replaces the file-static `Trajectory g_trajectory`, onedpath_ip.cpp:47-52)
 *   RP_VARIANT_F4  same spline, 4 multipliers, c_i = (a^2 - L^2)/2
 *                  (replaces `Trajectory2 g_trajectory`, onedpath2_ip.cpp:50-55)
 * Host-visible state is the reference's own array-of-structs layout, `double var[16]`
 * (enum V, onedpath_ip.cpp:15-43) or `double var[12]` (enum V2, onedpath2_ip.cpp:15-39)
 * per problem; on the device it is structure-of-arrays in the batch's compute type.
 *
 * Threading: a handle is not thread-safe (the reference is single-threaded: one GLUT
 * thread calls Problem::onKey).  Different handles may be used from different threads.
 * Batches that share a stream may be used from different threads too: the library takes a
 * per-stream lock for the length of each call.
 * Calls that enqueue work are asynchronous unless the doc says "synchronous"; rp_batch_sync()
 * waits.  They are ordered as if all of them ran on the batch's stream: that is where they run,
 * with one exception the caller cannot observe -- a fused rp_batch_solve that touches nothing
 * but memory the library owns may run on an auxiliary stream the library keeps beside the
 * batch's, so that back-to-back solves of DIFFERENT batches on one stream overlap (see
 * rp_solve_overlap_set for the rule).  Every other call on any batch of the stream, the stream
 * handle (rp_batch_stream), rp_batch_event_record and rp_batch_sync come after all of it.
 */
#ifndef RP_BATCH_H
#define RP_BATCH_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#if defined(__GNUC__)
#define RP_API __attribute__((visibility("default")))
#else
#define RP_API
#endif

typedef struct rp_batch rp_batch; /* opaque, owned by the caller between create and destroy */

/* ABI revision of this header: bumped whenever a struct that crosses the boundary changes size or an entry point changes
 * meaning.  rp_abi_version() returns what the LIBRARY was built with; a binding compares the two before its first call
 * (rocket_path_amd/capi.py and BatchedOneDPathIP do) -- rp_params grew in revision 2 (mu_mode, mu_sigma_try), and a caller
 * compiled against the older header would have handed rp_batch_set_params a shorter struct.
 *   1  round 1      2  round 2: rp_params + mu_mode / mu_sigma_try; rp_batch_field_ptr returns batch order (rp_batch_slot_map)
 *   3  round 3: sizeof(rp_params) returned by rp_params_size(); set_problems defers the feasible start
 *   4  round 4: rp_solution records (rp_batch_solution_device, rp_batch_bind_solution); rp_batch_traffic_probe replaces an
 *      environment switch; the library reads nothing from the environment; rp_batch_sample_device checks its alignment
 *   5  round 5: rp_device_id; a bound solution buffer is seeded before a gated launch that skips finished problems
 *   6  round 6: rp_pipeline_* (positions in -> solutions out over several streams); rp_params + handoff_rounds / handoff_lanes (the gated
 *      solve in rounds); a raw pointer to a mutable field keeps the seeding pass on for every later gated launch
 *   7  rp_batch_solution_vjp (gradients of the solution with respect to the positions); rp_batch_solution_jvp and
 *      rp_batch_solution_jacobian (the forward-mode derivative and the per-problem 3 x 3 Jacobian; new entries only);
 *      rp_batch_solution_hessian (the per-problem second derivatives; new entries only); rp_batch_set_problems_vel(_device),
 *      rp_batch_solution_vjp_vel, rp_batch_solution_jvp_vel and rp_batch_solution_jacobian_vel (problems with end velocities and the
 *      first derivatives in them; new entries only); rp_trajectory_eval, rp_trajectory_eval_vjp, rp_trajectory_eval_jvp and
 *      rp_batch_trajectory_device (a solved spline at the caller's own times, and the first derivatives of that evaluation; new entries
 *      only); rp_trajectory_crossing and rp_batch_crossing_device (the first time a spline reaches a level; new entries only: no
 *      struct changes size and no existing entry changes meaning, so the revision stays); rp_trajectory_extrema and
 *      rp_batch_extrema_device (the extreme position and velocity over a window of times; new entries only, the revision stays);
 *      rp_trajectory_gap (the extreme gap between two splines over a window of times; a new entry only, the revision stays);
 *      rp_trajectory_tracking, rp_trajectory_tracking_vjp and rp_trajectory_tracking_jvp (the integrals of the gap, its square and the
 *      square of its rate between two splines, with both derivative rules; new entries only, the revision stays);
 *      rp_trajectory_integrals, rp_trajectory_integrals_vjp, rp_trajectory_integrals_jvp and rp_batch_integrals_device (integrals over a
 *      window of times and their first derivatives; new entries only, the revision stays); rp_trajectory_eval_hvp (the second derivative
 *      of the evaluation along a direction; a new entry only, the revision stays); rp_trajectory_integrals_hvp (the second derivative of
 *      the integrals along a direction; a new entry only, the revision stays); rp_solve_overlap_set and rp_solve_overlap_stats
 *      (back-to-back fused solves of batches that share a stream overlap on an auxiliary stream; new entries only, no struct changes
 *      size and nothing a caller can observe through an existing entry changes, so the revision stays); rp_trajectory_meeting (the first
 *      time the gap between two splines reaches a level; a new entry only, the revision stays); rp_trajectory_tracking_hvp (the second
 *      derivative of the tracking integrals along a direction; a new entry only, the revision stays); rp_trajectory_separation (the
 *      closest approach of two vehicles moving in up to three axes; a new entry only, the revision stays); rp_trajectory_contact (the
 *      first time those two come within a distance; a new entry only, the revision stays); rp_trajectory_fleet_separation (that closest
 *      approach for every pair of a fleet in one launch; a new entry only, the revision stays); rp_trajectory_fleet_contact (that first time
 *      within a distance for every pair of a fleet in one launch; a new entry only, the revision stays);
 *      rp_trajectory_fleet_separation_staggered and rp_trajectory_fleet_contact_staggered (those two with a start time per vehicle; new
 *      entries only, the revision stays); rp_trajectory_fleet_reach, rp_trajectory_fleet_contact_culled(_workspace) and
 *      rp_trajectory_fleet_contact_candidates (the fleet's position boxes, and the fleet's first contacts with a broad phase that skips
 *      the pairs whose boxes prove them apart; new entries only, the revision stays); rp_trajectory_fleet_reach_staggered,
 *      rp_trajectory_fleet_contact_staggered_culled(_workspace) and rp_trajectory_fleet_contact_staggered_candidates (that broad phase
 *      with a start time per vehicle: a query is out when it is refused or box-far; new entries only, the revision stays);
 *      rp_trajectory_cross_separation and rp_trajectory_cross_contact (the two fleet queries for every vehicle of one fleet against every
 *      vehicle of another; new entries only, the revision stays) */
#define RP_ABI_VERSION 7

typedef enum {
    RP_OK = 0,
    RP_ERR_INVALID = 1,     /* bad argument (null handle, unknown variant/dtype, n == 0, ...) */
    RP_ERR_DEVICE = 2,      /* a HIP call failed; rp_last_error() has hipGetErrorString */
    RP_ERR_NOMEM = 3,       /* host or device allocation failed */
    RP_ERR_UNSUPPORTED = 4, /* valid request this build does not implement */
    RP_ERR_NO_DEVICE = 5    /* no HIP device visible: the product path has no CPU fallback */
} rp_status;

#define RP_VARIANT_F3 3
#define RP_VARIANT_F4 4
#define RP_DTYPE_F64 0
#define RP_DTYPE_F32 1
/* fp32 state in HBM (the traffic of RP_DTYPE_F32: 76 B per F4 step), fp64 arithmetic in registers; the state is
 * rounded to fp32 after every step.  One step from an fp32 state then agrees with the fp64 reference step from the
 * same state to fp32 rounding (6e-8 relative) for every problem, where pure fp32 arithmetic cannot: its Armijo test
 * (onedpath_ip.cpp:941) needs a relative residual decrease of 0.01 s, below fp32 resolution for s < 1e-5, and its 3x3
 * solve loses cond(K) * 6e-8 -- see DESIGN.md section 4, "Single precision". */
#define RP_DTYPE_F32_STATE 2

/* Per-problem status bits (new; the reference has no error reporting). */
#define RP_ST_CONVERGED 1u  /* gap < tol seen at a gate check */
#define RP_ST_MAXITER 2u    /* step cap reached before the gate */
#define RP_ST_NONFINITE 4u  /* a variable became NaN/inf */
#define RP_ST_INFEASIBLE 8u /* some c_i > 0 at the last gate check (constraintsSatisfied false) */
#define RP_ST_STALLED 16u   /* stall detector fired (only when rp_params.stall_window > 0); the problem is left alone from then on */
#define RP_ST_WRONG_WAY 32u /* with the stall detector on: a gated launch left the problem unconverged with a total duration no smaller than
                               the one it started the launch with -- F4's "settles the wrong direction" (README.md:34).  Cleared again
                               should a later launch converge the problem */

/* Solver constants, defaults = the reference's compile-time values. */
typedef struct {
    double accel_limit;       /* 100.0   onedpath_ip.cpp:54 */
    double mu_divisor;        /* 10.0    perturbation = gap / (m * 10), onedpath_ip.cpp:812 */
    double boundary_fraction; /* 0.99    onedpath_ip.cpp:915 */
    double backtrack;         /* 0.5     onedpath_ip.cpp:927, 944 */
    double armijo;            /* 0.01    onedpath_ip.cpp:941 */
    int32_t max_backtracks;   /* 100     onedpath_ip.cpp:919, 934 */
    int32_t stall_window;     /* 0 = off (the reference's behaviour: it keeps stepping, e.g. from initStuck, onedpath_ip.cpp:177-199).
                                 w > 0: in a gated solve, a problem whose surrogate gap has not halved for w consecutive steps of
                                 one launch is marked RP_ST_STALLED and stops -- SURVEY.md 8f row 4; never changes a converging run */
    int32_t mu_mode;          /* 0 = the reference's centring, perturbation = gap / (m * mu_divisor) at every step (onedpath_ip.cpp:812); the
                                 default, and the only mode the parity guarantees are about.
                                 1 = centring by trial (a Mehrotra-style predictor/centring split): the step is
                                 d_a + p d_c from one factorisation; sigma = mu_sigma_try[0], then [1] (p = sigma * gap / m) is taken if its
                                 full step keeps the multipliers positive, is primal feasible and passes the reference's residual test,
                                 else the reference step.  Same optimum in fewer steps (15.4 -> 12.7 mean on the benchmark distribution);
                                 double arithmetic only */
    double mu_sigma_try[2];   /* 0.01, 0.03 */
    int32_t handoff_rounds;   /* How the fused gated solve (rp_batch_solve with steps_per_launch <= 0) treats states its internal order says
                                 nothing about -- states that were set, nudged, moved or handed out raw since the last set_problems / init
                                 (reference mode only: mu_mode 0, no stall detector).
                                 0 (default): such a batch runs the kernel that WATCHES FOR FIXED POINTS: a problem whose step leaves
                                 its state bit for bit unchanged -- a start outside the feasible set: 100 feasibility halvings, no
                                 movement, onedpath_ip.cpp:919-928 -- takes its remaining step budget as read; count, status and state are
                                 exactly what stepping on would leave, without the ~20,000 evaluations.  Everything else (and the
                                 benchmark's path: set_problems -> solve) runs the plain kernel.
                                 2..8: additionally IN ROUNDS: a wave runs until its slowest lane is done, so one problem that needs 60
                                 steps holds 63 finished neighbours; in rounds a wave whose stepping lanes have numbered <= handoff_lanes
                                 for more than one step stops and leaves them open, the next launch packs all open problems densely,
                                 the last round runs to the end.  Same steps per problem, same results.  Pays only where most lane-steps
                                 would idle (measured: profiles/r6_state_families.log); costs 10-30 % where they would not.
                                 -1: the plain kernel always. */
    int32_t handoff_lanes;    /* 24 (1..48) */
} rp_params;

/* Batch-wide reduction, the payload of the one cross-GPU collective (max / max / sum / sum). */
typedef struct {
    double max_residual_sq; /* max_i ||r_i||^2 with r as residual(), onedpath_ip.cpp:753-792, p = gap_i/(10 m) */
    double max_gap;         /* max_i surrogateDualityGap, onedpath_ip.cpp:794-808 */
    double n_converged;     /* problems with RP_ST_CONVERGED (double so one dtype all-reduces) */
    double total_steps;     /* Newton steps executed since the last init/set_state */
} rp_reduction;

/* One problem's answer: what the reference leaves in var[vel1X], var[duration0], var[duration1] of its Trajectory
 * (onedpath_ip.cpp:47-52, read by printState 997-1006), plus the two progress words.  32 bytes = one HBM sector. */
typedef struct {
    double vel1, duration0, duration1;
    int32_t iters;   /* Newton steps taken since the last init / set_state / set_problems (gated + ungated) */
    uint32_t status; /* RP_ST_* */
} rp_solution;

/* ---- library ---- */
RP_API const char *rp_version(void);
RP_API int rp_abi_version(void);       /* RP_ABI_VERSION of the library's own build */
RP_API size_t rp_params_size(void);    /* sizeof(rp_params) in the library: must equal the caller's */
RP_API const char *rp_last_error(void); /* thread-local text of the last failure */
RP_API const char *rp_status_string(int status);
RP_API int rp_device_count(int *count);
/* "pci <domain:bus:device.function> uuid <hex>" of HIP device `device` into out (len >= 64).  New -- the reference is one process
 * on no device; a multi-GPU host (bench.py, ShardedOneDPathIP) reports with it that its N shards really sat on N different GPUs. */
RP_API int rp_device_id(int device, char *out, size_t len);
RP_API void rp_params_default(rp_params *p);

/* ---- lifetime ---- */
/* `stream` is a hipStream_t the caller owns (e.g. torch's current stream), the stream of another batch (rp_batch_stream), or NULL for
 * a stream the batch creates.  `device` is the HIP device ordinal.  A stream a batch created lives until the last batch on it has
 * been destroyed: the batch that created it may be destroyed before or after the batches that borrowed it.  Work the caller itself
 * enqueues on the stream is ordered after every library call made before it, except that fused solves still running on the
 * auxiliary stream (rp_solve_overlap_set) may not have finished: they touch no memory the caller can reach, and every call that
 * hands anything out waits for them. */
RP_API int rp_batch_create(rp_batch **out, int variant, int dtype, size_t n, int device, void *stream);
RP_API int rp_batch_destroy(rp_batch *b);
RP_API int rp_batch_set_params(rp_batch *b, const rp_params *p);
RP_API int rp_batch_get_params(const rp_batch *b, rp_params *p);
RP_API int rp_batch_size(const rp_batch *b, size_t *n);
RP_API int rp_batch_info(const rp_batch *b, int *variant, int *dtype, int *device);

/* ---- init: Problem::init() / onKey('i') / onKey('j') for every problem of the batch ---- */
RP_API int rp_batch_init_default(rp_batch *b); /* initDefault, onedpath_ip.cpp:201-228 / onedpath2_ip.cpp:164-193 */
RP_API int rp_batch_init_stuck(rp_batch *b);   /* initStuck, onedpath_ip.cpp:177-199 (F3 only) */
/* Per-problem positions (host arrays of n doubles), then the feasible start rule of
 * SURVEY.md 8d on the device: vel = 0, t_i = (3.5/sqrt 12) sqrt(6 |dX_i| / L), multipliers 1.
 * This (and rp_batch_set_state) is also where the batch decides in which order it keeps its problems internally
 * (sorted by expected step count, for the gated solve); callers never see that order except through
 * rp_batch_field_ptr: problem i of every call below is the problem of element i of these arrays. */
RP_API int rp_batch_set_problems(rp_batch *b, const double *pos0, const double *pos1, const double *pos2);
/* Same with device-resident inputs (no PCIe in the path).  Asynchronous: the three arrays are read, in the batch's stream order,
 * by this call's kernels only (they are copied), so they may be overwritten by later work on that stream.  The call computes the
 * batch's internal order and stops there: the start state itself is formed in registers by a fused rp_batch_solve
 * (steps_per_launch <= 0) that follows, or written out by whichever other call touches the state first -- same bits either way.
 * What a caller can observe of the deferral: "positions in, solutions out" costs one launch of state traffic less; the start
 * is the one of rp_params.accel_limit AS IT WAS when the problems were set (rp_batch_set_params writes the start out before
 * it changes the limit); raw pointers from rp_batch_field_ptr are undefined until the next state-touching call. */
RP_API int rp_batch_set_problems_device(rp_batch *b, const double *d_pos0, const double *d_pos1, const double *d_pos2);
/* Problems with non-zero end velocities (vel0X, vel2X of enum V): positions and velocities in PROBLEM order, device memory, n doubles
 * each; a NULL velocity array counts as zeros.  Every variant and dtype.  The scheduling pass of rp_batch_set_problems_device runs on
 * the positions, then one kernel writes the start -- not deferred -- with the velocities gathered into their fields (stored in the
 * batch's type, the start computed from the stored values):
 *     vel1 = 0, multipliers 1,  t_0 = (3.5/sqrt 12) sqrt(6 |dX_0| / L) + 8 |vel0| / L,  t_1 = (3.5/sqrt 12) sqrt(6 |dX_1| / L) + 8 |vel2| / L
 * -- rp_batch_set_problems_device's start bit for bit where the velocities are 0, and strictly feasible for any velocities (every
 * |a| <= 0.98 L).  The Newton kernels then run their general form (bit-identical to the zero-velocity form where the
 * velocities are 0), and the fused gated solve its watched kernel (the scheduled order was fitted to rest-to-rest starts): for zero or
 * NULL velocities iteration counts, status words and state are those of rp_batch_set_problems_device.  rp_batch_restart returns to this
 * start with the velocities the batch holds; a later rp_batch_set_problems(_device) zeroes them again.
 * The reference's F3 has no t > 0 constraint, and its backtracking can step over the t = 0 wall when the velocities are large: with
 * velocities kappa U(-1, 1) sqrt(L |dX|), 100 % of problems converge at kappa = 0.1, 99 % at 0.3, 81 % at 0.5 and 50 % at 1; the others
 * drift to negative or huge durations, and the status bits report them as for any problem (RP_ST_MAXITER, RP_ST_NONFINITE ...).  This
 * is the reference model's behaviour, reproduced.  Asynchronous, with rp_batch_set_problems_device's rules for the input arrays. */
RP_API int rp_batch_set_problems_vel_device(rp_batch *b, const double *d_pos0, const double *d_pos1, const double *d_pos2,
                                            const double *d_vel0, const double *d_vel2);
/* The same from host arrays.  Synchronous. */
RP_API int rp_batch_set_problems_vel(rp_batch *b, const double *pos0, const double *pos1, const double *pos2, const double *vel0,
                                     const double *vel2);
/* Back to the feasible start of the positions the batch already holds (the `I` key for per-problem positions): nothing
 * crosses the boundary.  Asynchronous.  A batch whose problems were set by rp_batch_set_problems_vel(_device) returns to that start,
 * with the end velocities it holds; every other batch to rest-to-rest (velocities zeroed). */
RP_API int rp_batch_restart(rp_batch *b);
/* Whole state in the reference's AoS layout, n * 16 (F3) or n * 12 (F4) doubles.  Synchronous. */
RP_API int rp_batch_set_state(rp_batch *b, const double *aos);
RP_API int rp_batch_get_state(rp_batch *b, double *aos);
/* The same for problems [first, first + count): count * 16 (or 12) doubles.  No per-call allocation and only the
 * requested rows cross PCIe -- what a host that watches ONE problem of the batch calls (printState, onedpath_ip.cpp:997-1006). */
RP_API int rp_batch_get_state_range(rp_batch *b, size_t first, size_t count, double *aos);
/* Special-key nudges (onSpecialKey, onedpath_ip.cpp:280-324): var[index] += delta for all problems. */
RP_API int rp_batch_nudge(rp_batch *b, int var_index, double delta);

/* ---- the hot path ---- */
/* k times onKey('n') = moveInteriorPoint (onedpath_ip.cpp:810-953 / onedpath2_ip.cpp:698-841)
 * on every problem, ungated, fused into one launch (state stays in registers between steps). */
RP_API int rp_batch_step(rp_batch *b, int k);
/* Diagnostic twin of rp_batch_step: the same k steps (same arithmetic: results are bit-identical to rp_batch_step's, state and
 * multipliers, for every k, variant and number mode -- every fixed-step kernel of a variant evaluates the reference's
 * post-convergence residual loop in the same form), returning per problem how often the feasibility loop
 * (onedpath_ip.cpp:927) and the residual loop (:944) halved the step over those k steps.  For decision-level comparisons with the
 * reference; one problem per lane, synchronous, not a fast path. */
RP_API int rp_batch_step_counted(rp_batch *b, int k, uint32_t *feas_halvings, uint32_t *resid_halvings);
/* Gated solve, the convention of SURVEY.md appendix A.5 per problem:
 *     for (it = 0; it < max_iter; ++it) { if (gap < gap_tol) break; step; }
 * steps_per_launch <= 0: one fused launch (each lane loops until its own gate);
 * steps_per_launch = s > 0: launches of s steps until every problem is done (host polls a
 * device counter after each launch; synchronous).  Iteration counts accumulate across calls
 * until the next init/set_state. */
RP_API int rp_batch_solve(rp_batch *b, double gap_tol, int max_iter, int steps_per_launch);
/* ONE asynchronous launch of up to k gated steps per still-open problem, no host polling: the building block of a solve
 * whose convergence check is global (multi-GPU: launch on every shard, all-reduce the summaries, repeat -- SURVEY.md 8d, C4;
 * rocket_path_amd/sharding.py, solve_with_global_checks). */
RP_API int rp_batch_solve_launch(rp_batch *b, double gap_tol, int max_iter, int k);
/* The Space key, moveTowardFeasibility (onedpath_ip.cpp:648-721), on every problem. */
RP_API int rp_batch_move_toward_feasibility(rp_batch *b);

/* ---- results ---- */
RP_API int rp_batch_get_iters(rp_batch *b, int32_t *iters, uint32_t *status); /* either may be NULL; synchronous */
/* Solutions in PROBLEM order in DEVICE memory the caller owns (n records, 32-byte aligned): record i is problem i of the arrays
 * handed to set_problems / set_state, whatever order the batch keeps internally -- the device-side counterpart of reading
 * var[] of trajectory i in the reference (onedpath_ip.cpp:47-52, 997-1006); nothing crosses PCIe.  Asynchronous on the batch
 * stream; works on any state (after steps, solves, nudges).  68 B of HBM traffic per problem. */
RP_API int rp_batch_solution_device(rp_batch *b, rp_solution *d_out);
/* Bind (NULL: unbind) a buffer of n records: from now on every gated solve (rp_batch_solve, rp_batch_solve_launch) writes the
 * record of each problem it works on as that problem leaves the launch -- "positions in, solutions out in problem order" then
 * costs no extra pass (the one 32-byte sector per problem is written under the solve's arithmetic).  After a gated solve of a
 * batch EVERY record is current, also those of problems that had finished in an earlier launch and that this one skipped: a
 * launch that may skip problems is preceded by one pass that writes all records from the state as it is (k_solution, 68 B per
 * problem) whenever the buffer is new or anything but gated solves has touched the state since the records were written; the
 * first solve of a batch that has just been given its problems stores every record itself and needs no such pass.  Calls other
 * than gated solves (rp_batch_step, nudges, set_state ...) do not update the buffer -- use rp_batch_solution_device for the
 * state they leave.  The buffer must outlive the binding. */
RP_API int rp_batch_bind_solution(rp_batch *b, rp_solution *d_out);
/* Vector-Jacobian product of the solution with respect to the positions, at the batch's current state (the
 * Newton matrix of onedpath_ip.cpp:814-861 transposed).  All arrays: n doubles, device memory, PROBLEM order; a NULL upstream
 * gradient counts as zeros.  Asynchronous on the batch stream.  F3, RP_DTYPE_F64 only (RP_ERR_UNSUPPORTED otherwise).
 * Definition: z = (x, lam), x = (vel1, duration0, duration1) with the 8 multipliers, theta = (pos0, pos1, pos2); r(z; theta, p) is
 * the reference's residual (onedpath_ip.cpp:753-783) with the perturbation p = gap / (m mu_divisor) of the state held fixed, and
 * M = dr/dz.  Given upstream gradients g on x: solve M^T w = [g; 0_8], theta_bar = -w^T dr/dtheta -- the implicit-function derivative
 * of the central-path point at this p, which tends to the derivative of the optimum as the gap goes to 0 wherever that exists.
 * r depends on theta only through pos1 - pos0 and pos2 - pos1, so pos0_bar + pos1_bar + pos2_bar = 0.  A problem whose state is
 * not finite or outside the feasible set (some c_i > 0, constraintsSatisfied of onedpath_ip.cpp:738-751: the states RP_ST_NONFINITE
 * and RP_ST_INFEASIBLE describe, judged from the state itself at the time of the call) gets NaN in all three outputs; every other
 * problem gets the formula, RP_ST_MAXITER ones included (|c_i| floored at L eps / 256 where rounding leaves an active c_i at 0).  Works on any state: after solves, steps, nudges, set_state, and on a
 * batch from rp_pipeline_batch. */
RP_API int rp_batch_solution_vjp(rp_batch *b, const double *d_g_vel1, const double *d_g_dur0, const double *d_g_dur1,
                                 double *d_pos0_bar, double *d_pos1_bar, double *d_pos2_bar);
/* Jacobian-vector product of the solution with respect to the positions, at the batch's current state: the
 * forward-mode counterpart of rp_batch_solution_vjp, with the same z, x, theta, r and M.  Given position tangents theta_dot =
 * (pos0_dot, pos1_dot, pos2_dot): solve M z_dot = -(dr/dtheta) theta_dot and write the x part (vel1_dot, duration0_dot,
 * duration1_dot).  All arrays: n doubles, device memory, PROBLEM order; a NULL tangent counts as zeros.  Equal tangents on the
 * three positions give exactly 0.  Asynchronous on the batch stream.  F3, RP_DTYPE_F64 only (RP_ERR_UNSUPPORTED otherwise).  The
 * NaN rule, the c_i floor and the states it works on are rp_batch_solution_vjp's. */
RP_API int rp_batch_solution_jvp(rp_batch *b, const double *d_t_pos0, const double *d_t_pos1, const double *d_t_pos2,
                                 double *d_t_vel1, double *d_t_dur0, double *d_t_dur1);
/* Every problem's Jacobian J = d(vel1, duration0, duration1) / d(pos0, pos1, pos2) at the batch's current state: 9 doubles per
 * problem, row-major (J[a][b] = dx_a / dpos_b at d_jac[9 i + 3 a + b]), n x 9 doubles of device memory in PROBLEM order.  The
 * derivative of rp_batch_solution_jvp / rp_batch_solution_vjp (J theta_dot and J^T g), formed by one elimination on the two
 * position-delta directions; each row sums to 0 up to rounding.  Asynchronous on the batch stream.  F3, RP_DTYPE_F64 only
 * (RP_ERR_UNSUPPORTED otherwise); a problem whose state is not finite or outside the feasible set gets NaN in all nine entries;
 * works on the states rp_batch_solution_vjp does. */
RP_API int rp_batch_solution_jacobian(rp_batch *b, double *d_jac);
/* Every problem's second derivatives H[a][b][c] = d^2 x_a / dpos_b dpos_c of x = (vel1, duration0, duration1) at the batch's current
 * state: the second derivative of the implicit function z(theta) that r(z; theta, p) = 0 defines, with the
 * z, x, theta, r and M of rp_batch_solution_vjp -- for tangents u, w, M z_uw = -R_uw, R_uw the second total derivative of r along
 * (z_u, u), (z_w, w) without the z_uw terms.  27 doubles per problem at d_hess[27 i + 9 a + 3 b + c], n x 27 doubles of device
 * memory in PROBLEM order, symmetric in (b, c); every row and column of each H[a] sums to 0 up to rounding.  d_jac may be NULL;
 * when given, it receives the Jacobian from the same first-order solves in rp_batch_solution_jacobian's layout (n x 9 doubles).
 * Asynchronous on the batch stream.  F3, RP_DTYPE_F64 only (RP_ERR_UNSUPPORTED otherwise); a problem whose state is not finite or
 * outside the feasible set gets NaN in all 27 (and 9) entries; works on the states rp_batch_solution_vjp does. */
RP_API int rp_batch_solution_hessian(rp_batch *b, double *d_jac, double *d_hess);
/* The first derivatives in all five boundary inputs theta = (pos0, pos1, pos2, vel0, vel2) at the batch's current state (DESIGN.md
 * section 12): the z, x, r, p and M of rp_batch_solution_vjp, the same double-double condensed K, c_i floor and NULL handling, with
 * dr/dtheta widened by the two end velocities (each enters only its own segment's accelerations).  NaN as for rp_batch_solution_vjp,
 * and also for a state with a duration <= 0.  They work on any state, rest-to-rest batches included (d / d vel at vel = 0).  The
 * position outputs are those of rp_batch_solution_vjp / _jvp / _jacobian (the same device code).  All arrays device memory, PROBLEM
 * order; asynchronous on the batch stream; F3, RP_DTYPE_F64 only (RP_ERR_UNSUPPORTED otherwise).
 *   vjp_vel       theta_bar = J^T g for upstream gradients g on x (NULL: zeros), five arrays of n doubles
 *   jvp_vel       x_dot = J theta_dot for the five tangents (NULL: zeros), three arrays of n doubles
 *   jacobian_vel  J[a][b] = dx_a / dtheta_b at d_jac[15 i + 5 a + b], b over (pos0, pos1, pos2, vel0, vel2): n x 15 doubles */
RP_API int rp_batch_solution_vjp_vel(rp_batch *b, const double *d_g_vel1, const double *d_g_dur0, const double *d_g_dur1,
                                     double *d_pos0_bar, double *d_pos1_bar, double *d_pos2_bar, double *d_vel0_bar, double *d_vel2_bar);
RP_API int rp_batch_solution_jvp_vel(rp_batch *b, const double *d_t_pos0, const double *d_t_pos1, const double *d_t_pos2,
                                     const double *d_t_vel0, const double *d_t_vel2, double *d_t_vel1, double *d_t_dur0, double *d_t_dur1);
RP_API int rp_batch_solution_jacobian_vel(rp_batch *b, double *d_jac);
RP_API int rp_batch_reduce(rp_batch *b, rp_reduction *out);                   /* synchronous */
/* Writes the 4 doubles of rp_reduction to device memory the caller owns, asynchronously on
 * the batch stream: the buffer a multi-GPU caller hands to its RCCL all-reduce. */
RP_API int rp_batch_reduce_device(rp_batch *b, double *d_out4);
/* For single-process multi-GPU hosts (csrc/host/sharded_problem.cpp): the same reduction into the batch's OWN
 * 4-double device slot, whose address is returned (asynchronous; all-reduce it in place on rp_batch_stream()),
 * and the synchronous read-back of that slot afterwards. */
RP_API int rp_batch_summary_device(rp_batch *b, double **d_out4);
RP_API int rp_batch_summary_read(rp_batch *b, rp_reduction *out);
/* Plot data (plotTrajectory/plotAcceleration, onedpath_ip.cpp:1015-1088): per problem 66
 * positions (33 per segment) and 4 end accelerations, host arrays, synchronous. */
RP_API int rp_batch_sample(rp_batch *b, double *pos66, double *acc4);

/* The same into DEVICE memory the caller owns (n x 66 and n x 4 doubles), asynchronously on the batch stream: for a consumer
 * that draws from device memory, and what bench.py times (nothing crosses PCIe). */
/* d_pos66 must be 16-byte aligned (positions are written as 16-byte vectors): RP_ERR_INVALID otherwise. */
RP_API int rp_batch_sample_device(rp_batch *b, double *d_pos66, double *d_acc4);

/* ---- a solved spline at the caller's own times (new: the reference only draws it, drawSegment, onedpath_ip.cpp:1065-1088) ----
 * Position, velocity and acceleration of the two-segment spline at k times per problem, and the first derivatives of that evaluation
 * (DESIGN.md section 13).  Stateless: any spline, not only a batch's.  The spline comes as a table of eight pointers to n doubles of
 * device memory each, in this order wherever such a table appears:
 *     (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1)
 * -- d_spline[3] and [4] (the end velocities) may be NULL: zeros.  d_tau holds the k query times of every problem, n x k doubles,
 * row-major, counted from the start of segment 0; every per-query array has that shape.
 * Segment rule: a query with tau < duration0 lies in segment 0, (pos0, vel0) -> (pos1, vel1) over h = duration0 at s = tau; every other
 * one in segment 1, (pos1, vel1) -> (pos2, vel2) over h = duration1 at s = tau - duration0.  With (x0, va) -> (x1, vb) the segment's ends:
 *     acc0 = 6 (x1 - x0) / h^2 - (4 va + 2 vb) / h        jrk0 = 2 (vb - va) / h^2 - 2 acc0 / h
 *     pos = x0 + (va + (acc0 + jrk0 s / 3) s / 2) s       vel = va + (acc0 + jrk0 s / 2) s       acc = acc0 + jrk0 s
 * (the cubic of onedpath_ip.cpp:1065-1088; divisions as refined reciprocals, the arithmetic of rp_batch_sample_device).  acc jumps at
 * the knot as the model's does; derivatives there are the selected segment's.
 * Extrapolation rule: no clamping -- outside [0, duration0 + duration1] the end segments' cubics continue.
 * NaN rule: a problem with a duration that is not finite or not > 0 gets NaN in all its outputs (rp_batch_solution_vjp_vel's rule); a
 * NaN tau gives NaN for that query only (in the VJP, the sums of its problem are NaN with it).
 * A NULL output is not wanted and costs no traffic; at least one must be given.  Every n x k array must be 16-byte aligned (the queries
 * move as 16-byte vectors), n and k positive, k < 2^31: RP_ERR_INVALID otherwise, as for a NULL required pointer, before any device
 * call.  `stream` is a hipStream_t of `device`, NULL the device's null stream.  Asynchronous; never throws. */
RP_API int rp_trajectory_eval(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_tau,
                              double *d_pos, double *d_vel, double *d_acc);
/* Reverse mode: upstream gradients on pos, vel, acc (n x k each; NULL: zeros, not read -- the same bits as explicit zeros) in, the
 * gradients of the eight spline inputs (n doubles each, the table's order; any entry, or the table, NULL: not wanted) and of tau
 * (n x k; NULL: not wanted) out.  Per query tau_bar = g_pos vel + g_vel acc + g_acc jrk0; per problem the k queries reduce to nine
 * sums in an order that depends on k alone -- no atomics: a problem's gradient is the same bits in a batch of 1 and of 2^20, and from
 * run to run -- and the chain rule through (acc0, jrk0) runs once.  pos1_bar and vel1_bar collect both segments;
 * duration0_bar also -(the sum of tau_bar over segment 1's queries). */
RP_API int rp_trajectory_eval_vjp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_tau,
                                  const double *d_g_pos, const double *d_g_vel, const double *d_g_acc,
                                  double *const d_spline_bar[8], double *d_tau_bar);
/* Forward mode, the transpose, pointwise: tangents on the eight spline inputs (any entry, or the table, NULL: zeros) and on tau
 * (NULL: zeros) in, tangents of pos, vel, acc out (NULL: not wanted; at least one). */
RP_API int rp_trajectory_eval_jvp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_tau,
                                  const double *const d_spline_dot[8], const double *d_tau_dot,
                                  double *d_pos_dot, double *d_vel_dot, double *d_acc_dot);
/* Second order: the derivative of rp_trajectory_eval_vjp's outputs (spline_bar[8], tau_bar) along the direction (spline_dot, tau_dot),
 * the upstream gradients held fixed -- S_o g_o (the second derivative of o) (spline_dot, tau_dot) over the outputs o of pos, vel, acc
 * (DESIGN.md section 17).  That matrix is symmetric: the one entry is forward-over-reverse and the (spline, tau) part of
 * reverse-over-reverse; the part of a double backward in the upstream gradients is rp_trajectory_eval_jvp.  The derivatives at a query are
 * the selected segment's, as everywhere.  Rules as rp_trajectory_eval_vjp's and _jvp's: any d_g_* NULL: zeros, not read; any entry of
 * d_spline_dot, the table, or d_tau_dot NULL: zeros, not read (NULL and explicit zeros give the same bits); any output NULL: not wanted,
 * not written, at least one given; every n x k array 16-byte aligned.  The k queries reduce as rp_trajectory_eval_vjp's do, in an order
 * that depends on k alone, no atomics: a problem's result is the same bits in any batch and from run to run.  NaN rule: a problem with a
 * duration that is not finite or not > 0 is NaN in all its outputs; a NaN tau or tau_dot makes its own tau_bar_dot NaN, and the sums of
 * its problem with it. */
RP_API int rp_trajectory_eval_hvp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_tau,
                                  const double *d_g_pos, const double *d_g_vel, const double *d_g_acc,
                                  const double *const d_spline_dot[8], const double *d_tau_dot,
                                  double *const d_spline_bar_dot[8], double *d_tau_bar_dot);
/* The arbitrary-time sibling of rp_batch_sample_device: rp_trajectory_eval of the batch's current state, PROBLEM order, every variant
 * and dtype (the state read in the batch's storage type, evaluated in double: bit for bit rp_trajectory_eval on what
 * rp_batch_get_state returns).  d_tau and the outputs: n x k doubles, 16-byte aligned, with rp_trajectory_eval's segment, extrapolation,
 * NaN and NULL rules.  Asynchronous on the batch stream; works on any state. */
RP_API int rp_batch_trajectory_device(rp_batch *b, const double *d_tau, size_t k, double *d_pos, double *d_vel, double *d_acc);

/* ---- the first time a spline reaches a level (new: the reference only draws the curve, drawSegment, onedpath_ip.cpp:1065-1088; replaces
 * a root search in the caller around rp_trajectory_eval, one launch per iteration) ----
 * d_level holds k levels per problem, n x k doubles row-major; d_time[i, j] becomes the earliest tau in [0, duration0 + duration1] with
 * pos(tau) = d_level[i, j] -- pos the cubic of rp_trajectory_eval, segment rule included -- and d_vel[i, j] (NULL: not wanted, not written)
 * the velocity there: rp_trajectory_eval's vel expression at the returned time.  d_time is required.  No extrapolation: a level the spline
 * does not reach on [0, duration0 + duration1] gives NaN in both outputs.
 * Piece rule: the roots of a segment's velocity strictly inside (0, h) cut it into at most three monotone pieces; the query takes the first
 * of the problem's six pieces, in time order, whose end positions hold the level between them.  A level equal to the position at the
 * start of its piece gives that breakpoint itself (level == pos0: 0.0 exactly); otherwise pos(s) = level is solved inside the piece by
 * Newton steps kept in a shrinking bracket (bisection where a step leaves it), until the residual is exactly zero or the step or the
 * bracket is below 2 ulp of the piece's end.  The trip count is bounded by a compile-time constant (64) for every input.
 * NaN rule: rp_trajectory_eval's -- a duration that is not finite or not > 0 makes every query of its problem NaN; a NaN (or infinite)
 * level gives NaN for that query only.  A level within rounding of an extremum of pos (a tangential touch) may come out as the touch, as a
 * later crossing, or as NaN.
 * Derivatives need no entry of their own: d time = (d level - d pos at fixed time) / vel, so reverse mode is one
 * rp_trajectory_eval_vjp launch with g_pos = -g / vel at the returned times, forward mode one rp_trajectory_eval_jvp launch.
 * Argument rules are rp_trajectory_eval's: d_spline[3] and [4] may be NULL (zeros), every n x k array 16-byte aligned, n and k positive,
 * k < 2^31; RP_ERR_INVALID before any device call otherwise.  Asynchronous on `stream`; never throws.  Pointwise: a query's bits depend on
 * its problem's eight numbers and its level only. */
RP_API int rp_trajectory_crossing(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_level,
                                  double *d_time, double *d_vel);
/* rp_trajectory_crossing of the batch's current state, PROBLEM order, every variant and dtype (the state read in the batch's storage
 * type, the search in double: bit for bit rp_trajectory_crossing on what rp_batch_get_state returns; replaces reading the state back
 * and searching on the host).  Asynchronous on the batch stream; works on any state. */
RP_API int rp_batch_crossing_device(rp_batch *b, const double *d_level, size_t k, double *d_time, double *d_vel);

/* ---- how far and how fast at most: the extreme position and velocity of a spline over a window of times (new: the reference only draws
 * the curve, drawSegment, onedpath_ip.cpp:1065-1088; replaces a dense grid of times through rp_trajectory_eval and a reduction over it) ----
 * Inputs: the spline, the table's order, the cubic, the segment rule (tau < duration0 selects segment 0) and the per-problem NaN rule are
 * rp_trajectory_eval's.  T = duration0 + duration1, the float64 sum.
 * Windows: query (i, j) has the window [lo, hi]; d_lo and d_hi are n x k doubles, row-major, 16-byte aligned.  A NULL d_lo counts as
 * -inf, a NULL d_hi as +inf; +-inf are allowed values.  No extrapolation: the window is clamped, a = lo > 0 ? lo : +0.0 and
 * b = hi < T ? hi : T (a NaN end stays NaN).  If !(a <= b) -- a NaN end, a window wholly outside [0, T], a problem under the NaN rule --
 * every output of the query is NaN.
 * Outputs: two tables of four pointers in the order (pos_min, pos_max, vel_min, vel_max): d_value[f] the extreme value on [a, b],
 * d_time[f] a time at which it is attained, each n x k.  A NULL entry (or a NULL table) is not wanted and costs no traffic; at least one
 * of the eight must be given.
 * Candidates, in time order: a; the interior candidates strictly inside (a, b) -- for position the real roots of each segment's velocity
 * strictly inside (0, h), for velocity each segment's s = -acc0 / jrk0 strictly inside (0, h) (jrk0 == 0 or anything not finite: none);
 * a segment-1 candidate's time is duration0 + s --; the knot duration0 if a <= duration0 <= b, for position too: a non-monotone optimum
 * has vel1 equal to 0 or to rounding, its velocity root then sits on s = 0 or s = h, which is not strictly inside, and without the knot
 * pos0 = 0, pos1 = 100, pos2 = 0, vel1 = 0 would have the maximum 0; and b.
 * Value and selection: every candidate's value is rp_trajectory_eval's at the candidate's time, so a returned value is bit for bit what
 * rp_trajectory_eval gives at the returned time.  The extreme is chosen by strict comparison along the candidates in time order: among
 * equal values the earliest time wins; a NaN candidate is skipped.
 * Returned time bits: the candidate's own -- a returns lo's bits (+0.0 when clamped), b returns hi's (T's when clamped), the knot
 * duration0's, a stationary point s or duration0 + s -- so that a caller can tell the candidates apart by equality.
 * Derivatives need no entry of their own: at a stationary candidate the value does not move with the time (the
 * envelope theorem), at the others the time is one of the inputs, so reverse mode is one rp_trajectory_eval_vjp launch at the returned
 * times with tau_bar routed to lo, hi, the durations or nowhere, forward mode one rp_trajectory_eval_jvp launch.
 * Not here: acceleration -- linear in each segment, its extremes are the four end accelerations the constraints already bound.
 * Argument rules are rp_trajectory_crossing's: d_spline[3] and [4] may be NULL (zeros), every given n x k array 16-byte aligned, n and k
 * positive, k < 2^31; RP_ERR_INVALID before any device call otherwise, also when all eight outputs (or both tables) are NULL.
 * Asynchronous on `stream`; never throws.  No loop whose trip count depends on data.  Pointwise: a query's bits depend on its problem's
 * eight numbers and its two window ends only. */
RP_API int rp_trajectory_extrema(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo,
                                 const double *d_hi, double *const d_value[4], double *const d_time[4]);
/* rp_trajectory_extrema of the batch's current state, PROBLEM order, every variant and dtype (the state read in the batch's storage type,
 * evaluated in double: bit for bit rp_trajectory_extrema on what rp_batch_get_state returns; replaces reading the state back and
 * scanning a grid on the host).  Asynchronous on the batch stream; works on any state. */
RP_API int rp_batch_extrema_device(rp_batch *b, const double *d_lo, const double *d_hi, size_t k, double *const d_value[4],
                                   double *const d_time[4]);

/* How much: the integrals of the spline of rp_trajectory_eval over windows of time (replaces a dense grid through
 * rp_trajectory_eval summed on the host or in torch -- k times the traffic, an answer as good as the grid, and a wrong gradient of |vel| near
 * its sign changes -- and Gauss points placed by hand).  The spline, the order of the eight-pointer table, the cubic, the segment constants
 * and the per-problem NaN rule are rp_trajectory_eval's; the windows are rp_trajectory_extrema's: d_lo and d_hi n x k, a NULL d_lo counts as
 * -inf and a NULL d_hi as +inf, infinite values allowed; a = lo > 0 ? lo : +0.0, b = hi < T ? hi : T with T = duration0 + duration1 the
 * double sum, a NaN end stays NaN; unless a <= b every output of the query is NaN; if a == b every output is exactly +0.0.
 * Outputs: one table of four pointers in the order (pos_int, distance, vel_sq, acc_sq), each n x k: the integrals over [a, b] of pos, of
 * |vel| (the distance actually travelled: the sum of |pos increment| over the monotone pieces the roots of the velocity strictly inside a
 * segment cut it into, clipped to the window), of vel^2 and of acc^2.  A NULL entry is not wanted and costs no traffic (and the distance,
 * the expensive one, no work); at least one must be given.  Each output is the sum of the two segments' contributions, segment 0's
 * (if a < duration0, over [a, min(b, duration0)]) first, then segment 1's (if b > duration0): acc jumps at the knot and the window is
 * split there.
 * Arithmetic: each contribution is a polynomial in the piece's length, taken from the global ends, with coefficients from pos, vel, acc at
 * the piece's start; no antiderivative is differenced, so a window of 1e-9 T late in a segment keeps its digits.
 * Argument rules are rp_trajectory_extrema's: d_spline[3] and [4] may be NULL (zeros), every given n x k array 16-byte aligned, n and k
 * positive, k < 2^31; RP_ERR_INVALID before any device call otherwise, also when all four outputs (or the table) are NULL.
 * Asynchronous on `stream`; never throws.  No loop whose trip count depends on data.  Pointwise: a query's bits depend on its problem's
 * eight numbers and its two window ends only. */
RP_API int rp_trajectory_integrals(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo,
                                   const double *d_hi, double *const d_value[4]);
/* Reverse mode of rp_trajectory_integrals (replaces differentiating the grid sum or the hand-placed Gauss points through a dozen elementwise
 * launches whose `where` chains give NaN gradients on the branches not taken): for upstream gradients d_g[4] on the four outputs (n x k each;
 * a NULL entry or table: zeros, the same bits as explicit zeros; a query whose outputs are NaN counts as zeros), the gradients in the eight
 * spline inputs d_spline_bar[8] (n each, the table's order) and in the window's ends d_lo_bar, d_hi_bar (n x k).  A NULL output is not wanted
 * and not written; at least one must be given.  The derivative is that of the branch the forward took: an end's term goes to lo_bar where
 * a = lo, nowhere where a is the clamp +0.0, to hi_bar where b = hi, to the durations where b = T, to duration0_bar where a segment ends or
 * starts on the knot's side of a window that crosses it (DESIGN.md section 16 has the table and the kinks at ties).
 * A problem's gradient is the same bits alone and in a batch of any size, and from run to run: rp_trajectory_eval_vjp's order of additions
 * (a function of k alone), no atomics.  Argument rules as above. */
RP_API int rp_trajectory_integrals_vjp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo,
                                       const double *d_hi, const double *const d_g[4], double *const d_spline_bar[8], double *d_lo_bar,
                                       double *d_hi_bar);
/* Forward mode of rp_trajectory_integrals (replaces the same torch compositions under forward_ad): tangents on the eight spline inputs
 * d_spline_dot[8] (n each) and on the window's ends d_lo_dot, d_hi_dot (n x k) in -- any of them NULL: zeros, the same bits as explicit zeros
 * --, the tangents of the wanted outputs d_value_dot[4] out (NaN where the output is).  Pointwise; the same routing of the ends as the
 * reverse mode.  Argument rules as above. */
RP_API int rp_trajectory_integrals_jvp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo,
                                       const double *d_hi, const double *const d_spline_dot[8], const double *d_lo_dot, const double *d_hi_dot,
                                       double *const d_value_dot[4]);
/* Second order of rp_trajectory_integrals (replaces differencing rp_trajectory_integrals_vjp along the direction --
 * two launches, a step to choose, half the digits -- and makes torch.autograd.functional.hvp / hessian and Newton or Gauss-Newton outer
 * loops on effort, distance and mean-position losses possible at all): the derivative of rp_trajectory_integrals_vjp's ten outputs
 * (d_spline_bar[8], d_lo_bar, d_hi_bar) along the direction (d_spline_dot[8], d_lo_dot, d_hi_dot) with the upstream gradients d_g[4] held
 * fixed, that is (sum over the four outputs o of g_o x the second derivative of o) x the direction.  The matrix is symmetric: the one entry
 * is forward-over-reverse and the (spline, lo, hi) part of reverse-over-reverse; the part of a double backward in d_g is
 * rp_trajectory_integrals_jvp.  The derivative is that of the formulas rp_trajectory_integrals_vjp evaluates on the branch the forward
 * took: which end is lo, hi or a clamp, which segment contributes and whether segment 0 ends on the knot or at b are held fixed (a second
 * derivative is one-sided at section 16's ties).  Exact: the four integrals are polynomials in the segment constants and the local ends.
 * The distance's second derivative is concentrated on the sign changes of the velocity: a root c of a segment's velocity strictly inside
 * the clipped piece adds 2 g_distance vel_dot(c) / |acc(c)| x (1, c, c^2 / 2) to the dotted partials in (va, acc0, jrk0), with vel_dot the
 * direction's velocity at fixed local time; a touch (acc(c) == 0 exactly) adds nothing, and there is no guard otherwise: near a double root
 * the term is large because the function is like that there (a factor that is not finite counts as 0).  The sign of the velocity at an end
 * of a piece is taken from inside the piece -- the segment's first sign, turned once per root passed -- not from the end's own velocity,
 * which is rounding at a rest-to-rest spline's own ends: along directions that keep the end velocities (the solve's duration tangents
 * included) the result is the two-sided derivative there; along one that moves a zero end velocity the distance's is one-sided.
 * A NULL d_g entry or table, a NULL entry of d_spline_dot, the whole table, d_lo_dot or d_hi_dot: zeros, the same bits as explicit zeros (a
 * NULL d_g[1] also costs no walk over the monotone pieces).  A NULL output is not wanted and not written; at least one must be given.  A
 * query whose outputs are NaN counts with gradients of zero and gets lo_bar_dot = hi_bar_dot = 0 -- also in a problem under the per-problem
 * NaN rule (rp_trajectory_integrals_vjp's convention), which is NaN in its eight per-problem outputs only; a NaN d_lo_dot (d_hi_dot) on an
 * end that is taken makes its own query's lo_bar_dot (hi_bar_dot) and the sums of its problem that its segment reaches NaN, not the other
 * end's output (the mixed derivative in the two ends is zero); on a clamped end it is not read.  A problem's bits depend on its own inputs and on k only -- rp_trajectory_eval_vjp's order of additions, no atomics.
 * Argument rules as above.  Asynchronous on `stream`; never throws. */
RP_API int rp_trajectory_integrals_hvp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo,
                                       const double *d_hi, const double *const d_g[4], const double *const d_spline_dot[8],
                                       const double *d_lo_dot, const double *d_hi_dot, double *const d_spline_bar_dot[8], double *d_lo_bar_dot,
                                       double *d_hi_bar_dot);
/* rp_trajectory_integrals of the batch's current state, PROBLEM order, every variant and dtype (the state read in the batch's storage type,
 * evaluated in double: bit for bit rp_trajectory_integrals on what rp_batch_get_state returns; replaces reading the state back and summing
 * a grid on the host).  Asynchronous on the batch stream; works on any state. */
RP_API int rp_batch_integrals_device(rp_batch *b, const double *d_lo, const double *d_hi, size_t k, double *const d_value[4]);

/* ---- how close two splines get: the extreme gap between two splines in one frame over a window of times (new: the
 * reference draws one curve, drawSegment, onedpath_ip.cpp:1065-1088; replaces a dense grid of times through rp_trajectory_eval on both
 * splines -- k times the traffic, an answer as good as the grid -- and two rp_trajectory_extrema calls, which bound the gap but do not
 * give it) ----
 * Inputs: spline A and spline B, each the eight pointers of rp_trajectory_eval in its table's order, with its cubic, its segment rule and
 * its per-problem NaN rule: if either spline is under the rule every output of the problem is NaN.  T_A and T_B are the float64 sums
 * duration0 + duration1.
 * Queries: query (i, j) has a window [lo, hi] and a delay: B's clock starts `delay` after A's, B is at t - delay when A is at t.  d_lo,
 * d_hi and d_delay are n x k doubles, row-major, 16-byte aligned.  A NULL d_lo counts as -inf, a NULL d_hi as +inf, a NULL d_delay as 0;
 * +-inf window ends are allowed; a NaN or infinite delay makes the query's outputs NaN.
 * Gap: D(t) = pos_A(t) - pos_B(t - delay), pos the evaluator's.  No extrapolation: the common domain is [S, E], S = delay > 0 ? delay :
 * +0.0, E = min(T_A, delay + T_B) with delay + T_B the float64 sum delay + (duration0_B + duration1_B), T_A among equals.  The window is
 * clamped, a = lo > S ? lo : S and b = hi < E ? hi : E (a NaN end stays NaN); if !(a <= b) every output of the query is NaN.
 * Knots and pieces: k_A = duration0_A and k_B = delay + duration0_B (the float64 sum), walked in time order, k_A first among equals; those
 * that lie in [a, b] cut it into at most three pieces.  On a piece with left end c, A is in segment 1 if k_A <= c (local time c - k_A,
 * else c) and B if k_B <= c (local time c - k_B, else c - delay); the relative velocity is a quadratic in u = t - c whose constants are
 * the difference of the two segments' (vel, acc, jrk0) at c, its roots those of rp_trajectory_crossing's quadratic formula.  A root is a
 * candidate if it is strictly inside (0, the piece's length) and its time c + u strictly inside (a, b); the smaller root first.
 * Candidates, in time order: a; piece 0's roots; the first knot if it lies in [a, b]; piece 1's roots; the second knot if it lies in
 * [a, b]; piece 2's roots; b.
 * Value and selection: every candidate's value is the float64 difference of rp_trajectory_eval's pos of A at the candidate's time and of
 * B at time - delay (the float64 difference), so a returned value is bit for bit rp_trajectory_eval(A, time) - rp_trajectory_eval(B,
 * time - delay).  The extreme is chosen by strict comparison along the candidates in time order, as rp_trajectory_extrema's: among equal
 * values the earliest time wins; a NaN candidate is skipped.
 * Outputs: two tables of two pointers in the order (gap_min, gap_max): d_value[f] the extreme gap on [a, b], d_time[f] a time (on A's
 * clock) at which it is attained, each n x k.  A NULL entry (or table) is not wanted and costs no traffic; at least one of the four must be
 * given.  Returned time bits: the candidate's own -- a returns lo's bits, or delay's or +0.0 when clamped; b returns hi's, or T_A's or
 * the sum delay + T_B's when clamped; a knot k_A's or k_B's; a root the sum c + u -- so that a caller can tell the candidates apart by
 * equality.  The unsigned separation of the two is clamp(max(gap_min, -gap_max), min = 0).
 * Derivatives need no entry of their own: reverse mode is one rp_trajectory_eval_vjp launch on each spline at the
 * returned times (B's minus the delay), forward mode one rp_trajectory_eval_jvp launch on each, with the derivative in the time routed to
 * lo, hi, the delay, the durations, or nowhere (a stationary point: the envelope theorem).
 * There is no batch entry: two batches would multiply the storage-type x variant x zero-velocity dispatch to 64 forms.
 * Argument rules are rp_trajectory_extrema's: entries [3] and [4] of either table may be NULL (zeros), every given n x k array 16-byte
 * aligned, n and k positive, k < 2^31; RP_ERR_INVALID before any device call otherwise, also when all four outputs (or both tables) are
 * NULL.  Asynchronous on `stream`; never throws.  No loop whose trip count depends on data.  Pointwise: a query's bits depend on its
 * problem's sixteen numbers and its own window ends and delay only. */
RP_API int rp_trajectory_gap(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8],
                             const double *d_lo, const double *d_hi, const double *d_delay, double *const d_value[2], double *const d_time[2]);

/* ---- how far apart two splines are on average: the tracking integrals between two splines in one frame over a window of times (DESIGN.md
 * section 20; new: the reference draws one curve; replaces a dense grid of times through rp_trajectory_eval on both splines -- k times the
 * traffic, an answer as good as the grid, a dozen elementwise launches in each derivative mode; rp_trajectory_integrals of either spline
 * alone does not hold the cross term of the squared gap, and rp_trajectory_gap is a maximum, not an average) ----
 * Inputs, queries, the gap D, the common domain [S, E], the clamped window [a, b], the knots k_A and k_B and the segment each spline is in
 * on a piece are rp_trajectory_gap's, word for word.  The two knots, in time order with k_A first among equals and each clamped into
 * [a, b], leave three pieces [c, e], some of length zero; on a piece A's local start is s_A = c - k_A in segment 1, else c, and B's is
 * s_B = c - k_B in segment 1, else c - delay.
 * Per piece: X, V, A are the float64 differences of the two selected segments' pos, vel, acc at their local starts in the evaluator's
 * expressions, J that of their jrk0, w = e - c from the GLOBAL ends, and with third = 1.0 / 3.0
 *     gap_int   = w (X + (w / 2) (V + (w third) (A + (w / 4) J)))
 *     gap_sq    = w (X X + w (X V + w t3)),  t3 = (V V + X A) third + w t4,  t4 = (V A + (X J) third) / 4 + w t5,
 *                 t5 = ((A A) / 4 + (V J) third) / 5 + w t6,  t6 = (A J) / 36 + w ((J J) / 252)
 *     relvel_sq = w (V V + w (V A + (w third) ((A A + V J) + w (0.75 (A J) + (0.15 w) (J J)))))
 * (divisions by constants are multiplications by the rounded reciprocals 0.5, 0.25, 0.2, 1.0 / 36.0, 1.0 / 252.0; no contraction).
 * Outputs: a table of three pointers in the order (gap_int, gap_sq, relvel_sq), n x k each: the integrals over [a, b] of D, of D^2 and of
 * (dD/dt)^2, each the sum piece 0 + piece 1 + piece 2 in that order; exactly 0.0 where a == b; NaN where !(a <= b), where the delay is NaN
 * or infinite, and for a problem either of whose splines is under the NaN rule.  A NULL entry is not wanted and costs no traffic; at least
 * one must be given.
 * There is no batch entry (rp_trajectory_gap's reason).  Argument rules are rp_trajectory_gap's: entries [3] and [4] of either spline
 * table may be NULL (zeros), every given n x k array 16-byte aligned, n and k positive, k < 2^31; RP_ERR_INVALID before any device call
 * otherwise, also when no output is given.  Asynchronous on `stream`; never throws.  No loop whose trip count depends on data.  Pointwise:
 * a query's bits depend on its problem's sixteen numbers and its own window ends and delay only. */
RP_API int rp_trajectory_tracking(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8],
                                  const double *const d_spline_b[8], const double *d_lo, const double *d_hi, const double *d_delay,
                                  double *const d_value[3]);
/* The reverse rule of rp_trajectory_tracking (replaces a backward pass through the dense grid).  d_g: the three upstream gradients, n x k
 * each (NULL entries, or a NULL table: zeros).  Outputs, each optional (NULL: not formed): d_spline_a_bar and d_spline_b_bar, eight arrays
 * of n each in the spline table's order, and d_lo_bar, d_hi_bar, d_delay_bar, n x k; at least one must be given.  The derivative is that of
 * the formulas above on the branch the forward took, with every piece end's derivative sent to where the end came from (lo, hi, the delay,
 * the durations, or nowhere for the clamp +0.0).  A query whose outputs are NaN counts with upstream gradients of
 * zero (a problem under the NaN rule has NaN constants and NaN gradients).  One launch per spline, back to back on `stream` (side A's also forms the three per-query gradients; a side nothing is wanted of is
 * not launched).  The order of every addition is a function of k alone: a problem's gradient is the same bits in any batch; no atomics.
 * Argument rules as above. */
RP_API int rp_trajectory_tracking_vjp(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8],
                                      const double *const d_spline_b[8], const double *d_lo, const double *d_hi, const double *d_delay,
                                      const double *const d_g[3], double *const d_spline_a_bar[8], double *const d_spline_b_bar[8],
                                      double *d_lo_bar, double *d_hi_bar, double *d_delay_bar);
/* The forward rule (replaces a forward-mode pass through the dense grid): tangents on both splines' eight inputs (NULL entries or tables:
 * zeros) and on lo, hi and the delay (NULL: zeros) in, the three outputs' tangents out (NULL entries: not wanted; at least one), NaN where
 * the output is.  A NULL tangent counts as the value zero in the same expression: NULL and explicit zeros give the same bits.  Pointwise,
 * one launch.  Argument rules as above. */
RP_API int rp_trajectory_tracking_jvp(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8],
                                      const double *const d_spline_b[8], const double *d_lo, const double *d_hi, const double *d_delay,
                                      const double *const d_spline_a_dot[8], const double *const d_spline_b_dot[8], const double *d_lo_dot,
                                      const double *d_hi_dot, const double *d_delay_dot, double *const d_value_dot[3]);
/* Second order of rp_trajectory_tracking (replaces differencing rp_trajectory_tracking_vjp along the direction -- four
 * launches, a step to choose, half the digits -- and makes torch.autograd.functional.hvp / hessian and Newton or Gauss-Newton outer loops on
 * tracking and spacing losses possible): the derivative of rp_trajectory_tracking_vjp's nineteen outputs (d_spline_a_bar[8],
 * d_spline_b_bar[8], d_lo_bar, d_hi_bar, d_delay_bar) along the direction (d_spline_a_dot[8], d_spline_b_dot[8], d_lo_dot, d_hi_dot,
 * d_delay_dot) with the upstream gradients d_g[3] held fixed, that is (sum over the three outputs o of g_o x the second derivative of o) x
 * the direction.  The matrix is symmetric: the one entry is forward-over-reverse and the input part of reverse-over-reverse; the part of a
 * double backward in d_g is rp_trajectory_tracking_jvp.  The derivative is that of the formulas rp_trajectory_tracking_vjp evaluates on the
 * branch the forward took: the classes of a and b (lo / the START / the clamp +0.0; hi / END_A / END_B), the order of the two knots, which
 * knot is clamped to which end and the segment each spline is in on each piece are held fixed.  Every piece end is an affine function of
 * lo, hi, the delay and the durations with constant coefficients and carries rp_trajectory_tracking_jvp's tangent; at ties, and at a delay
 * of exactly 0, a second derivative is one-sided.  Exact: the three integrals are polynomials in the segment constants, the local piece
 * starts and the piece lengths; there is no root term and no division per query.
 * A NULL d_g entry or table, a NULL entry of either _dot table or a whole table, d_lo_dot, d_hi_dot or d_delay_dot: zeros, the same bits as
 * explicit zeros.  A NULL output is not formed; at least one must be given.  A query whose outputs are NaN counts with gradients of zero; a
 * problem either of whose splines is under the NaN rule is NaN in its sixteen per-problem results, and its per-query results are 0 or NaN
 * where rp_trajectory_tracking_vjp's are.  A NaN d_lo_dot (d_hi_dot) on an end that is clamped is not read.  One launch per spline, back to
 * back on `stream` (side A's also forms the three per-query results; a side nothing is wanted of is not launched).  A problem's bits depend
 * on its own inputs and on k only -- rp_trajectory_eval_vjp's order of additions, no atomics, no loop whose trip count depends on data.
 * Argument rules as above.  Asynchronous on `stream`; never throws. */
RP_API int rp_trajectory_tracking_hvp(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8],
                                      const double *const d_spline_b[8], const double *d_lo, const double *d_hi, const double *d_delay,
                                      const double *const d_g[3], const double *const d_spline_a_dot[8], const double *const d_spline_b_dot[8],
                                      const double *d_lo_dot, const double *d_hi_dot, const double *d_delay_dot,
                                      double *const d_spline_a_bar_dot[8], double *const d_spline_b_bar_dot[8], double *d_lo_bar_dot,
                                      double *d_hi_bar_dot, double *d_delay_bar_dot);

/* ---- when two splines meet: the first time in a window at which the gap between two splines reaches a level (new:
 * the reference draws one curve; the inverse of rp_trajectory_gap's D as rp_trajectory_crossing is of rp_trajectory_eval's pos; replaces a
 * root search on the host around two rp_trajectory_eval calls -- two launches per iteration and no derivative through the root) ----
 * Inputs, queries, the gap D(t) = pos_A(t) - pos_B(t - delay), the common domain [S, E], the clamped window [a, b], the knots k_A and k_B
 * (k_A first among equals) and the per-problem NaN rule are rp_trajectory_gap's, word for word; a NaN or infinite delay, or !(a <= b),
 * makes the query NaN.  d_level, n x k doubles: the level of each query; NULL counts as 0 (the two at the same position); a NaN or
 * infinite level makes its own query NaN.
 * The meeting time is the earliest t in [a, b] with D(t) = level, on A's clock; NaN if the gap does not reach the level in the window (no
 * extrapolation).  Sub-pieces: rp_trajectory_gap's up to three pieces, each cut at its candidate roots of the relative velocity (the same
 * roots by the same tests, the smaller first; a root that is no candidate leaves a sub-piece of length zero): nine monotone sub-pieces
 * between ten breakpoints in time order -- a, roots, knot, roots, knot, roots, b; a knot outside [a, b] is the end it is clamped to.  Each
 * breakpoint's gap is rp_trajectory_eval(A, t) - rp_trajectory_eval(B, t - delay), computed once.  The query takes the first sub-piece
 * whose two end values hold the level between them, inclusive, in either direction (a NaN fails).  If the level equals the value at the
 * sub-piece's start the time is that breakpoint with its own bits (lo's, delay's, +0.0, k_A's, k_B's, or a root's sum c + u).  Otherwise
 * D(c + u) = level is solved by rp_trajectory_crossing's search -- secant start, Newton steps kept in the bracket and bisected where
 * they leave it or fail to halve the step before last, until g == 0, the bracket or the step is within 2 ulp of the sub-piece's later end
 * (as a time on A's clock), or one step after a Newton step whose own error estimate is; the point of smallest |g| seen; at most 64
 * trips, whatever the input -- on the piece's local cubic: (X, V, A, J) the differences of the two selected segments' pos, vel, acc and
 * jrk0 at the piece's start c, u = t - c; the time is c + u, kept inside the sub-piece's two ends.
 * Outputs: d_time (required) and d_relvel (NULL: not wanted), n x k each.  d_relvel is the closing velocity at the returned time, bit for
 * bit vel of rp_trajectory_eval(A, time) minus vel of rp_trajectory_eval(B, time - delay), NaN exactly where the time is.
 * A level within rounding of an extreme of D in the window may come out as the touch, as a later meeting, or as NaN
 * (rp_trajectory_crossing's rule).
 * Derivatives need no entry of their own: D(theta_A, theta_B, t, delay) = level gives d time = (d level - d pos_A
 * + d pos_B - vel_B(time - delay) d delay) / relvel -- one rp_trajectory_eval_vjp or _jvp launch on each spline.
 * There is no batch entry (rp_trajectory_gap's reason).  Argument rules are rp_trajectory_gap's: entries [3] and [4] of either spline
 * table may be NULL (zeros), every given n x k array 16-byte aligned, n and k positive, k < 2^31, d_time not NULL; RP_ERR_INVALID before
 * any device call otherwise.  Asynchronous on `stream`; never throws.  Pointwise: a query's bits depend on its problem's sixteen numbers
 * and its own level, window ends and delay only. */
RP_API int rp_trajectory_meeting(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8],
                                 const double *const d_spline_b[8], const double *d_level, const double *d_lo, const double *d_hi,
                                 const double *d_delay, double *d_time, double *d_relvel);

/* ---- how close two vehicles moving in several axes get: the least squared distance over a window and when it is attained (DESIGN.md
 * section 24; new: the reference draws one curve.  A vehicle in the plane or in space is d splines, one per axis, solved as d independent
 * problems; the closest approach is no function of rp_trajectory_gap's per-axis extremes, which are attained at different times) ----
 * d: the number of axes, 1, 2 or 3.  d_spline_a, d_spline_b: tables of 8 d pointers, axis-major -- entries [8 c .. 8 c + 7] are axis c's
 * spline in rp_trajectory_eval's order, with its cubic, its segment rule and its NaN rule; if any of the 2 d splines of a problem is
 * under the NaN rule, every output of that problem is NaN.  Queries are rp_trajectory_gap's: d_lo, d_hi, d_delay, n x k doubles each (NULL
 * counts as -inf, +inf, 0); vehicle B is at t - delay when A is at t, one delay for all axes; a NaN or infinite delay makes the query NaN.
 * D_c(t) = pos_Ac(t) - pos_Bc(t - delay) and the value is f(t) = the sum over c of D_c(t)^2, the SQUARED distance (smooth where the
 * vehicles touch).  No extrapolation: the common domain is [S, E] with S = delay > 0 ? delay : +0.0 and E the smallest of the 2 d ends T_Ac
 * and delay + T_Bc (A's before B's and a lower axis first among equals); the window is clamped to [a, b] inside it as rp_trajectory_gap
 * clamps, and !(a <= b) makes the query NaN.
 * Pieces: the 2 d knots k_Ac = duration0_Ac and k_Bc = delay + duration0_Bc cut [a, b] into at most 2 d + 1 pieces, walked without sorting:
 * a piece ends at the smallest knot greater than its start and smaller than b, else at b.  On a piece with start c and u = t - c,
 * g(u) = f'(u) / 2 = the sum of D_c(u) D_c'(u) is a quintic whose coefficients come from each axis' (X, V, A, J), the differences of the two
 * selected segments' pos, vel, acc and jrk0 at c.  Its roots with a change of sign are isolated by the derivative chain -- the roots of g'''
 * in closed form bracket those of g'', those the roots of g', those the roots of g -- and each bracket whose end values differ in sign is
 * solved by rp_trajectory_crossing's kind of search (secant start, Newton steps kept in the bracket and bisected where they leave it or
 * fail to halve the step before last, until p == 0 or the bracket or the step is within 2 ulp of the piece's end as a time on A's clock;
 * the point of smallest |p| seen; at most 64 trips, whatever the input).  Nothing divides by a leading coefficient.
 * Candidates in time order: a; per piece the roots of g strictly inside the piece and strictly inside (a, b), as times c + u, then the knot
 * that ends it; b.  Each candidate's value is the sum, in axis order, of the squares of pos of rp_trajectory_eval(A_c, t) minus pos of
 * rp_trajectory_eval(B_c, t - delay), plain products and sums -- a returned value is bit for bit that expression at the returned time.
 * The least value wins, the earliest among equals; a NaN never.
 * Outputs, n x k each, either may be NULL but not both: d_value, the least squared distance; d_time, when it is attained, on A's clock,
 * with its candidate's own bits (lo's, delay's, +0.0, hi's, the winning end's, a knot's, or a root's sum c + u).
 * Derivatives need no entry of their own: the envelope theorem, one rp_trajectory_eval_vjp or _jvp launch per spline
 * at the returned time.  There is no batch entry (rp_trajectory_gap's reason).  Argument rules are rp_trajectory_gap's: entries [3] and [4]
 * of any axis may be NULL (zeros), every given n x k array 16-byte aligned, n and k positive, k < 2^31; d outside 1..3, a NULL table or
 * both outputs NULL give RP_ERR_INVALID before any device call.  Asynchronous on `stream`; never throws.  Pointwise: a query's bits depend
 * on its problem's 16 d numbers and its own window ends and delay only. */
RP_API int rp_trajectory_separation(int device, void *stream, size_t n, size_t k, int d, const double *const *d_spline_a,
                                    const double *const *d_spline_b, const double *d_lo, const double *d_hi, const double *d_delay,
                                    double *d_value, double *d_time);

/* ---- when two vehicles moving in several axes first come within a distance (new: the reference draws one curve) ----
 * The inverse of rp_trajectory_separation: d, the two tables of 8 d pointers, the NaN rule over the 2 d splines, the queries d_lo, d_hi and
 * d_delay with their NULL meanings, D_c(t), f(t) = the sum over c of D_c(t)^2, the domain [S, E], the clamped window [a, b], the 2 d knots and
 * the unsorted walk of 2 d + 1 pieces are that entry's, word for word.  d_level_sq, n x k doubles, required: the level of each query in units
 * of SQUARED distance, like that entry's value (a radius r is the level r r); a NaN or infinite level makes its own query NaN; a negative one
 * is legal and never reached.  d_time, n x k, required: the earliest t in [a, b] with f(t) = level, on A's clock; NaN where f does not reach
 * the level in the window (no extrapolation).
 * Each piece [c, e] is cut at the sign-changing roots of its quintic f' / 2 that are rp_trajectory_separation's candidates (the same
 * coefficients, the same chain, the same stopping width 2 ulp of e; a root that is no candidate repeats the breakpoint before it), six
 * sub-pieces on which f is monotone.  A breakpoint's value is the sum, in axis order, of the squares of pos of rp_trajectory_eval(A_c, t)
 * minus pos of rp_trajectory_eval(B_c, t - delay), computed once: a level between f(a) and f(b) is held by some sub-piece's end values
 * whatever the rounding.  The first sub-piece, in time order, whose end values hold the level between them (inclusive, either direction; a
 * NaN holds nothing) gives the answer: its start with its own bits (lo's, delay's, +0.0, a knot's, a root's sum c + u) if the level equals
 * the value there; otherwise the root of (F0 - level) + the sum of g_i (2 / (i + 1)) u^(i + 1), f - level about c, by the chain's search
 * between the sub-piece's ends, as the time c + u kept inside the sub-piece (a level equal to the value at the end: that end, its bits).
 * A level within rounding of an extreme of f may come out as the touch, as a later contact or as NaN.
 * d_rate, n x k, may be NULL: f' at the returned time, bit for bit 2.0 times the sum in axis order from 0.0 of (pos_Ac - pos_Bc) (vel_Ac -
 * vel_Bc) on rp_trajectory_eval's outputs at t and t - delay; NaN exactly where the time is.
 * Derivatives need no entry of their own (section 25): dt = (dlevel - df at fixed t) / rate, one rp_trajectory_eval_vjp or _jvp launch per
 * spline at the returned time.  There is no batch entry (rp_trajectory_gap's reason).  Argument rules are rp_trajectory_separation's; d
 * outside 1..3, a NULL table, a NULL d_level_sq or d_time, a misaligned n x k array, n or k of 0 give RP_ERR_INVALID before any device
 * call.  Asynchronous on `stream`; never throws.  Pointwise: a query's bits depend on its problem's 16 d numbers and its own level, window
 * ends and delay only. */
RP_API int rp_trajectory_contact(int device, void *stream, size_t n, size_t k, int d, const double *const *d_spline_a,
                                 const double *const *d_spline_b, const double *d_level_sq, const double *d_lo, const double *d_hi,
                                 const double *d_delay, double *d_time, double *d_rate);

/* ---- the closest approach of every pair of a fleet, in one launch (new: the reference draws one curve) ----
 * n scenes of m vehicles each, 2 <= m <= 256, all vehicles of a scene on one clock.  d_fleet: ONE table of 8 d pointers, axis-major, in
 * rp_trajectory_separation's order; each array holds n m doubles, vehicle v of scene s at s m + v.  d_lo, d_hi: n x k doubles, the windows
 * of scene s for ALL its pairs (NULL: -inf, +inf); read as single values, no alignment rule.  pairs = m (m - 1) / 2, ordered (i, j), i < j,
 * lexicographic: (0, 1), (0, 2), .., (0, m - 1), (1, 2), ..  The outputs d_value and d_time are n x pairs x k, either may be NULL but not
 * both.  Output [s, (i, j), q] is what rp_trajectory_separation returns, bit for bit in value and time, for A = vehicle i of scene s,
 * B = vehicle j of scene s, the window [lo, hi][s, q] and d_delay == NULL: that entry's NaN rule (over the pair's 2 d splines: a vehicle
 * under it makes exactly its m - 1 pairs NaN), domain, candidates and earliest-among-equals.  No pair-expanded array is read or written:
 * the staging of a (scene, pair) problem reads the two vehicles where they lie.
 * Derivatives need no entry of their own (section 26): rp_trajectory_separation's routing per vehicle instead of per pair, one
 * rp_trajectory_eval and one rp_trajectory_eval_vjp or _jvp launch per axis on the n m splines.  There is no batch entry.  Entries [3] and
 * [4] of any axis may be NULL (zeros); the outputs 16-byte aligned; m outside 2..256, d outside 1..3, a NULL table, both outputs NULL,
 * n or k of 0, k >= 2^31 give RP_ERR_INVALID before any device call.  Asynchronous on `stream`; never throws.  Pointwise: a query's
 * bits depend on its two vehicles' 16 d numbers and its scene's window ends only. */
RP_API int rp_trajectory_fleet_separation(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                          const double *d_lo, const double *d_hi, double *d_value, double *d_time);

/* ---- the first contact of every pair of a fleet, in one launch (new: the reference draws one curve) ----
 * rp_trajectory_contact for every pair of rp_trajectory_fleet_separation's fleet: n, m, d, d_fleet, the order of the pairs, d_lo and d_hi
 * (n x k per scene, single values, no alignment rule, NULL: -inf, +inf) are that entry's, word for word.  d_level_sq, required, in units of
 * SQUARED distance like rp_trajectory_contact's, in one of two layouts: level_per_pair == 0: n x k doubles, one level for all pairs of
 * scene s at query q, read as single values where the window ends are, no alignment rule; level_per_pair == 1: n x pairs x k doubles in the
 * outputs' layout, read as 16-byte vectors and 16-byte aligned -- what vehicles of different sizes need, (r_i + r_j)^2 formed by the caller.
 * d_time, n x pairs x k, required; d_rate, the same shape, may be NULL.  Output [s, (i, j), q] is what rp_trajectory_contact returns, bit for
 * bit in time and rate, for A = vehicle i of scene s, B = vehicle j of scene s, the window [lo, hi][s, q], that query's level and
 * d_delay == NULL: that entry's NaN rule (over the pair's 2 d splines: a vehicle under it makes exactly its m - 1 pairs NaN), a NaN or
 * infinite level making its own query NaN and a negative one never reached, the sub-pieces, the early exit, the zero-length skip and the
 * rate.  No pair-expanded array of splines is read or written.
 * Derivatives need no entry of their own (section 27): rp_trajectory_contact's implicit-function formula routed per vehicle, one
 * rp_trajectory_eval and one rp_trajectory_eval_vjp or _jvp launch per axis on the n m splines.  There is no batch entry.  Entries [3] and
 * [4] of any axis may be NULL (zeros); m outside 2..256, d outside 1..3, a NULL table, level or time, a level_per_pair other than 0 or 1,
 * a misaligned output, a misaligned per-pair level, n or k of 0, k >= 2^31, an n x pairs x k that does not fit give RP_ERR_INVALID
 * before any device call.  Asynchronous on `stream`; never throws.  Pointwise: a query's bits depend on its two vehicles' 16 d numbers,
 * its level and its scene's window ends only. */
RP_API int rp_trajectory_fleet_contact(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                       const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi, double *d_time,
                                       double *d_rate);

/* ---- the vehicles of one fleet against the vehicles of another, in one launch (new entries only, the revision
 * stays) ----
 * n scenes; in each, m_a vehicles of fleet A and m_b of fleet B, 1 <= m_a, m_b <= 32768, all on one clock.  d_fleet_a and d_fleet_b: one
 * table of 8 d pointers each, axis-major, in rp_trajectory_separation's order; A's arrays hold n m_a doubles, vehicle v of scene s at
 * s m_a + v, B's n m_b, at s m_b + v.  pairs = m_a m_b, pair r = (i, j) = (r / m_b, r % m_b), vehicle i of A against vehicle j of B,
 * row-major: an n x pairs x k output is n x m_a x m_b x k.  No pair of two vehicles of the same fleet is looked at.  d_lo, d_hi: n x k
 * doubles, the windows of scene s for all its pairs (NULL: -inf, +inf), read as single values, no alignment rule.
 * rp_trajectory_cross_separation: d_value and d_time, n x pairs x k, either may be NULL but not both.  rp_trajectory_cross_contact:
 * d_level_sq, required, in rp_trajectory_fleet_contact's two layouts (level_per_pair == 0: n x k, single values, no alignment rule; 1:
 * n x pairs x k, 16-byte aligned -- (r_i + r_j)^2 for vehicles and obstacles of different sizes); d_time, n x pairs x k, required;
 * d_rate, the same shape, may be NULL.
 * Output [s, (i, j), q] is, bit for bit, what rp_trajectory_separation returns in value and time (rp_trajectory_contact in time and rate)
 * for A = vehicle i of scene s of fleet A, B = vehicle j of scene s of fleet B, the window [lo, hi][s, q], that query's level and
 * d_delay == NULL.  That entry's NaN rule carries over: a vehicle of A under it makes exactly its row of m_b pairs NaN, a vehicle of B
 * exactly its column of m_a pairs; so do its domain -- the common one, which ends with the shorter of the two total times: a vehicle that
 * stands still (an obstacle) needs durations that cover the window -- its candidates and its earliest-among-equals.  No pair-expanded
 * array is read or written.
 * Derivatives need no entry of their own (section 34): the fleet entries' formulas, a vehicle of A summing over its row and a vehicle of B
 * over its column, one rp_trajectory_eval and one rp_trajectory_eval_vjp or _jvp launch per axis and fleet.  There is no batch entry.
 * Entries [3] and [4] of any axis of either table may be NULL (zeros); m_a or m_b of 0 or above 32768, d outside 1..3, a NULL table, both
 * outputs NULL (separation), a NULL level or time (contact), a level_per_pair other than 0 or 1, a misaligned output, a misaligned
 * per-pair level, n or k of 0, k >= 2^31, an n x pairs x k that does not fit give RP_ERR_INVALID before any device call.  Asynchronous
 * on `stream`; never throws.  Pointwise: a query's bits depend on its two vehicles' 16 d numbers, its level and its scene's window ends
 * only. */
RP_API int rp_trajectory_cross_separation(int device, void *stream, size_t n, size_t m_a, size_t m_b, size_t k, int d,
                                          const double *const *d_fleet_a, const double *const *d_fleet_b, const double *d_lo,
                                          const double *d_hi, double *d_value, double *d_time);
RP_API int rp_trajectory_cross_contact(int device, void *stream, size_t n, size_t m_a, size_t m_b, size_t k, int d,
                                       const double *const *d_fleet_a, const double *const *d_fleet_b, const double *d_level_sq,
                                       int level_per_pair, const double *d_lo, const double *d_hi, double *d_time, double *d_rate);

/* ---- the two fleet queries with a start time per vehicle (new entries only, the revision stays) ----
 * d_start, required: n x m doubles, vehicle v of scene s at s m + v, read as single values, no alignment rule.  Vehicle v runs its spline
 * over [start, start + T] of the scene's clock; d_lo, d_hi (n x k, NULL: -inf, +inf) and d_time are on the scene's clock.  For pair (i, j),
 * i < j, with s_i and s_j the two starts: delay = s_j - s_i, lo' = lo - s_i, hi' = hi - s_i, one fp64 subtraction each (a NULL end is the
 * infinity before the subtraction).  Output [s, (i, j), q] is what rp_trajectory_separation (rp_trajectory_contact, at the same level)
 * returns, bit for bit in value, time and rate, for A = vehicle i, B = vehicle j, the window [lo', hi'] and that delay: d_time_local is
 * that entry's time t', on vehicle i's clock, and d_time is t' + s_i, one fp64 addition (NaN stays NaN).  So the pair entry's NaN rule (a
 * NaN or infinite start makes exactly that vehicle's m - 1 pairs NaN), common domain (pairs never under way together are NaN), candidates,
 * delayed start and earliest-among-equals hold.  Every other argument, the order of the pairs and every refusal are
 * rp_trajectory_fleet_separation's and rp_trajectory_fleet_contact's, except that any output may be NULL (d_value, d_time, d_time_local;
 * d_time, d_time_local, d_rate) but not all; a NULL d_start gives RP_ERR_INVALID, before any device call like the rest.  No pair-expanded
 * array is read or written: a query decodes its pair again and loads the two starts where they lie.  Asynchronous on `stream`; never
 * throws.  Pointwise: a query's bits depend on its two vehicles' 16 d numbers and starts, its level and its scene's window ends only. */
RP_API int rp_trajectory_fleet_separation_staggered(int device, void *stream, size_t n, size_t m, size_t k, int d,
                                                    const double *const *d_fleet, const double *d_start, const double *d_lo,
                                                    const double *d_hi, double *d_value, double *d_time, double *d_time_local);
RP_API int rp_trajectory_fleet_contact_staggered(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                                 const double *d_start, const double *d_level_sq, int level_per_pair, const double *d_lo,
                                                 const double *d_hi, double *d_time, double *d_time_local, double *d_rate);

/* ---- the fleet's first contacts with a broad phase in front (new entries only, the revision stays) ----
 * rp_trajectory_fleet_reach: for vehicle v of scene s, axis c and query q the least and greatest position of that spline over the scene's
 * window [lo, hi][s, q]: rp_trajectory_extrema's pos_min and pos_max of that spline and window, bit for bit -- its clamp to [0, T] and its
 * NaN for an empty clamped window and under the NaN rule.  n, m, k, d, d_fleet, d_lo and d_hi are rp_trajectory_fleet_separation's; d_min,
 * d_max: d pointers each, axis c's to n x m x k doubles, 16-byte aligned; a NULL table or entry is not written, at least one must be.
 *
 * rp_trajectory_fleet_contact_culled: rp_trajectory_fleet_contact's outputs, bit for bit in d_time and d_rate, NaN bits included, for
 * the same first thirteen arguments, which it refuses as that entry does and in its order.  In front of the search: the boxes above;
 * per pair and query a lower bound of the squared distance of the two vehicles' boxes, made smaller by a slack per vehicle and axis and
 * a margin (section 30 proves that a pair whose bound is above the level in all k queries has k NaN outputs); those pairs get the NaN
 * written directly and the search runs over the list of the others, so that the time goes with the number of pairs that are near and
 * not with m^2.  A NaN or infinite box end, slack or level keeps the pair.  Every element of d_time and d_rate is written exactly once.
 * d_workspace: caller-owned, 16-byte aligned, at least the bytes rp_trajectory_fleet_contact_culled_workspace gives for (n, m, k, d);
 * its contents before the call do not matter and after it are unspecified.  d_kept (n x pairs bytes: 1 the pair went to the search, 0 it
 * was culled), d_list (n x pairs uint32_t: the kept problems s pairs + pair in increasing order in its first *d_count entries, the rest
 * unspecified) and d_count (one uint32_t) are copies for callers and tests, NULL: not written; the host never reads them.  Beyond
 * rp_trajectory_fleet_contact's refusals: n x pairs >= 2^32, a NULL or misaligned workspace, workspace_bytes below the size asked for --
 * RP_ERR_INVALID before any device call.  No block of any of its kernels waits for another; no atomics: the same list and bits in every run.
 *
 * rp_trajectory_fleet_contact_candidates: the broad phase alone -- boxes, sieve, no search: d_kept, required, as above.
 * All asynchronous on `stream`; none throws. */
RP_API int rp_trajectory_fleet_reach(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                     const double *d_lo, const double *d_hi, double *const *d_min, double *const *d_max);
RP_API int rp_trajectory_fleet_contact_culled_workspace(size_t n, size_t m, size_t k, int d, size_t *bytes);
RP_API int rp_trajectory_fleet_contact_culled(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                              const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi,
                                              double *d_time, double *d_rate, void *d_workspace, size_t workspace_bytes,
                                              unsigned char *d_kept, uint32_t *d_list, uint32_t *d_count);
RP_API int rp_trajectory_fleet_contact_candidates(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                                  const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi,
                                                  void *d_workspace, size_t workspace_bytes, unsigned char *d_kept);

/* ---- that broad phase with a start time per vehicle (new entries only, the revision stays) ----
 * rp_trajectory_fleet_reach_staggered: rp_trajectory_fleet_reach with d_start (n x m, required, as rp_trajectory_fleet_contact_staggered's):
 * the window of vehicle v is taken on v's own clock, [lo - start_v, hi - start_v], one fp64 subtraction each (a NULL end is the infinity
 * before the subtraction), and the box is rp_trajectory_extrema's pos_min and pos_max of that spline over that window, bit for bit.
 *
 * rp_trajectory_fleet_contact_staggered_culled: rp_trajectory_fleet_contact_staggered's outputs, bit for bit in d_time, d_time_local and
 * d_rate, NaN bits included, for the same first fifteen arguments, which it refuses as that entry does and in its order (any output may
 * be NULL but not all).  In front of the search, per pair and query two tests: refused -- the query's window on the first vehicle's clock
 * does not meet the two vehicles' common domain, decided by the search's own fp64 operations on the same numbers, exactly -- or far --
 * the boxes above are further apart than the level, with section 30's slacks and margin and an allowance for the time error of the
 * second vehicle's clock (section 31 proves that either gives NaN outputs).  A pair whose k queries are each refused or far gets its NaN
 * written directly; the search runs over the list of the others.  A pair with a NaN or infinite start is kept; so is a query with a NaN or
 * infinite box end, slack, speed bound or total time that is not refused.  Every element of each non-NULL output is written exactly once.
 * d_workspace: as rp_trajectory_fleet_contact_culled's, of rp_trajectory_fleet_contact_staggered_culled_workspace's size; d_kept, d_list,
 * d_count and the refusals beyond rp_trajectory_fleet_contact_staggered's: as there, before any device call.  No block waits for another,
 * no atomics: the same list and bits in every run.
 *
 * rp_trajectory_fleet_contact_staggered_candidates: the broad phase alone -- boxes, the two tests, no search: d_kept, required.
 * All asynchronous on `stream`; none throws. */
RP_API int rp_trajectory_fleet_reach_staggered(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                               const double *d_start, const double *d_lo, const double *d_hi, double *const *d_min,
                                               double *const *d_max);
RP_API int rp_trajectory_fleet_contact_staggered_culled_workspace(size_t n, size_t m, size_t k, int d, size_t *bytes);
RP_API int rp_trajectory_fleet_contact_staggered_culled(int device, void *stream, size_t n, size_t m, size_t k, int d,
                                                        const double *const *d_fleet, const double *d_start, const double *d_level_sq,
                                                        int level_per_pair, const double *d_lo, const double *d_hi, double *d_time,
                                                        double *d_time_local, double *d_rate, void *d_workspace, size_t workspace_bytes,
                                                        unsigned char *d_kept, uint32_t *d_list, uint32_t *d_count);
RP_API int rp_trajectory_fleet_contact_staggered_candidates(int device, void *stream, size_t n, size_t m, size_t k, int d,
                                                            const double *const *d_fleet, const double *d_start, const double *d_level_sq,
                                                            int level_per_pair, const double *d_lo, const double *d_hi, void *d_workspace,
                                                            size_t workspace_bytes, unsigned char *d_kept);

/* The same as rp_batch_sample_device for problems [first, first + count) only (what onDraw needs for the watched problem). Synchronous. */
RP_API int rp_batch_sample_range(rp_batch *b, size_t first, size_t count, double *pos66, double *acc4);
/* The rest of printState for problems [first, first + count): `Surrogate gap` and the `Constraints:` table
 * (printConstraints, onedpath_ip.cpp:955-995, 1008-1010).  Per problem 1 + 14 m doubles (m = 8 for F3, 4 for F4):
 * [0] = surrogate gap; then for constraint i at 1 + 14 i: error, deriv[3], second[3][3] row-major, dot = (0,-1,-1).deriv.
 * Variable order (vel1X, duration0, duration1) as in enum V.  Synchronous. */
RP_API int rp_batch_constraints_range(rp_batch *b, size_t first, size_t count, double *rows);

/* ---- stream / timing plumbing ---- */
/* Bandwidth calibration: the one-launch-per-step kernel with NO step -- its loads and stores of every problem's state and
 * nothing else (the state is rewritten unchanged).  What bench.py prices the k = 1 launch against.  Asynchronous. */
RP_API int rp_batch_traffic_probe(rp_batch *b);
RP_API int rp_batch_sync(rp_batch *b);
RP_API int rp_batch_stream(rp_batch *b, void **stream);
/* Overlap of back-to-back fused solves of batches that share a stream (process-wide switch and counters; new entries only, the
 * revision stays).  A launch's wave slots empty out while its last chunks drain, and the next launch on the same stream waits for
 * the previous one to retire; a caller who solves batch after batch on ONE stream gets what a caller with two streams gets if
 * every second solve runs on an auxiliary stream the library keeps beside the caller's (one per stream and device, created at
 * the first solve that may overlap, destroyed with the last batch on the stream).
 * Which solves: rp_batch_solve in its fused form (steps_per_launch <= 0) as a single launch (not in rounds), of a batch with no
 * bound solution buffer, no raw pointer handed out (rp_batch_field_ptr), outside an rp_pipeline, and -- in mode 1 -- of at least
 * 65,536 problems.  Such a solve reads and writes nothing but memory the library owns.
 * The ordering rule: eligible solves that follow one another directly alternate between the caller's stream and the auxiliary
 * one.  The auxiliary stream waits, through an event recorded on the caller's stream, for everything the library enqueued there
 * before -- in particular for the last operation of the batch being solved; a solve on the caller's stream of a batch whose
 * previous solve ran on the auxiliary stream waits for that solve.  EVERY other call that takes a batch (set_problems, restart,
 * step, every read-back, reduce, the derivative and trajectory entries, rp_batch_event_record, rp_batch_sync, rp_batch_stream,
 * rp_batch_destroy ...) first makes the caller's stream wait for everything on the auxiliary one.  So consecutive solves of
 * different batches overlap pairwise, and whatever can be observed through this API or through the stream is ordered as before;
 * only the moment a solve's kernel runs relative to FOREIGN work on the stream is not, which no memory the caller owns depends on.
 * mode 0: off, every call runs on the batch's stream.  1 (default): automatic.  2: every eligible solve whatever its size (tests).
 * out[4]: solves sent to the auxiliary stream / solves kept on the caller's stream although eligible (alternation, or size in
 * mode 1) / joins enqueued / solves excluded by the list above.  Counted in modes 1 and 2 since the library was loaded. */
RP_API int rp_solve_overlap_set(int mode);
RP_API int rp_solve_overlap_stats(unsigned long long out[4]);
/* HIP events on the batch's own stream: record slot 0..7, elapsed between two recorded slots. */
RP_API int rp_batch_event_record(rp_batch *b, int slot);
RP_API int rp_batch_event_elapsed_ms(rp_batch *b, int slot_start, int slot_stop, float *ms);
/* Device pointer of one SoA field (0..15 / 0..11) for callers that manage their own copies.  Elements are in BATCH
 * order: the batch keeps its problems sorted for the gated solve (set_problems / set_state decide the order), problem i's
 * element is ptr[slot_of_problem[i]] with the map of rp_batch_slot_map.  Asking for an end-velocity field
 * (vel0X / vel2X) makes the batch assume they may become non-zero (general kernels) until the next init /
 * set_problems / set_state.  A pointer taken earlier is undefined between rp_batch_set_problems(_device) and the next call
 * that touches the state (the feasible start is written lazily): take it again after set_problems.  Once a pointer to a
 * CONSTANT field (positions, end velocities) has been handed out the batch assumes for the rest of its life that positions may be
 * written behind its back: rp_batch_sample_device then always reads them from the fields (the gather path), never from the
 * records set_problems kept. */
RP_API int rp_batch_field_ptr(rp_batch *b, int field, void **d_ptr);
/* slot_of_problem[i] = position of problem i inside the batch's field arrays (n words; the identity after
 * init_default / init_stuck).  Every other entry point takes and returns problem order; only rp_batch_field_ptr
 * exposes batch order.  Synchronous. */
RP_API int rp_batch_slot_map(rp_batch *b, uint32_t *slot_of_problem);

/* ---- positions in -> solutions out, batch after batch (new: the reference solves ONE problem per key press, onedpath_ip.cpp:269-272;
 * this is the caller either side of the batched path) ----
 * A pipeline owns `depth` batches of n problems on one device and `n_streams` (1..4, depth a multiple of it) streams; job i goes to
 * batch i % depth on stream (i % depth) % n_streams.  rp_pipeline_submit enqueues, for one job and without synchronising the host,
 * exactly what a caller would issue by hand -- rp_batch_bind_solution, rp_batch_set_problems_device (the scheduling pass),
 * rp_batch_solve (fused, from the feasible start formed in registers) -- so every result is bit for bit the one-stream path's.  What
 * the arrangement buys: with n_streams >= 2 the scheduling pass of job i + 1 (memory- and latency-bound) and the first waves of its
 * solve run under the drain of job i's solve (vector-ALU bound, wave slots emptying): "positions in, solutions out" at the rate of
 * the solve kernel alone or better (bench.py `end_to_end`).
 *   inputs_stream  the stream whose earlier work produces the position arrays (NULL: they are ready now); the job waits for it
 *                  on the device.  The arrays must stay untouched until the job's scheduling pass has read them:
 *                  rp_pipeline_stream_wait(job, 0, s) makes stream s wait for exactly that, rp_pipeline_wait(job) the host.
 *   d_out          n rp_solution records in problem order (32-byte aligned; NULL: none -- read the batch through rp_pipeline_batch)
 * (An application note, not something the library does: the HIP runtime maps a process's streams onto GPU_MAX_HW_QUEUES hardware
 * queues, and streams that share a queue serialise.  In a process that already owns two or three streams of its own the pipeline's two
 * streams may come to share a queue: 73 against 91 G Newton steps/s on one box, profiles/r6_hw_queues.log.)
 *   job            receives the job's number (0, 1, 2, ...); a slot is reused every `depth` jobs, in stream order -- the previous
 *                  job of the slot has finished on the device before the new one touches the batch; its d_out is the caller's to
 *                  have consumed by then. */
typedef struct rp_pipeline rp_pipeline;
RP_API int rp_pipeline_create(rp_pipeline **out, int variant, int dtype, size_t n, int device, int depth, int n_streams);
RP_API int rp_pipeline_destroy(rp_pipeline *p);
RP_API int rp_pipeline_set_params(rp_pipeline *p, const rp_params *params); /* every batch of the pipeline */
/* Where the scheduling pass of a job runs (before the first submit only).  INLINE (the default): on the job's own stream, ahead of its
 * solve.  STREAM / PRIORITY: on one more stream the pipeline owns (PRIORITY: created with the device's highest stream priority), ordered
 * behind the slot's previous job and ahead of the job's solve by events.  Measured equal to INLINE within 1 % where the process owns few
 * streams; every further stream risks sharing a hardware queue with another (the HIP runtime has GPU_MAX_HW_QUEUES = 4 of them by
 * default), and streams that share a queue serialise. */
#define RP_PIPELINE_PREP_INLINE 0
#define RP_PIPELINE_PREP_STREAM 1
#define RP_PIPELINE_PREP_PRIORITY 2
#define RP_PIPELINE_PREP_FAT_KERNELS 16 /* OR-ed in: keep the scheduling pass in its 256-thread form (A/B measurements; same order) */
RP_API int rp_pipeline_set_prep(rp_pipeline *p, int mode);
RP_API int rp_pipeline_submit(rp_pipeline *p, const double *d_pos0, const double *d_pos1, const double *d_pos2, rp_solution *d_out,
                              double gap_tol, int max_iter, void *inputs_stream, int64_t *job);
/* Host waits until job (and everything submitted to its slot before it) has finished; job < 0: everything submitted. */
RP_API int rp_pipeline_wait(rp_pipeline *p, int64_t job);
/* Device-side dependency: `stream` waits until the job's position arrays have been read (what = 0) or its solutions are
 * written (what = 1).  Only while the job is still the last one of its slot. */
RP_API int rp_pipeline_stream_wait(rp_pipeline *p, int64_t job, int what, void *stream);
/* The batch that holds job (while it is still the last one of its slot): every rp_batch_* read-back works on it (rp_batch_reduce,
 * rp_batch_get_iters, rp_batch_sample_device ...), on the job's own stream.  Owned by the pipeline. */
RP_API int rp_pipeline_batch(rp_pipeline *p, int64_t job, rp_batch **batch);

#ifdef __cplusplus
}
#endif
#endif
