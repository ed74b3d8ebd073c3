// ip_kernels.h -- host-callable launchers of the HIP kernels (internal; the public surface
// is include/rp_batch.h).  All launchers enqueue on `stream` and return the hipError_t of
// the launch; none synchronises.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stddef.h>
#include <stdint.h>

namespace rp {

// What the scheduling pass keeps per problem for a batch that has just been given its problems: 32 bytes, one sector.
struct StartRecord {
    double pos0, pos1, pos2;
    long long problem;      // the problem's own index (diagnostic; nothing on the path reads it)
};

// One problem's answer, 32 bytes = one sector (the layout of rp_solution in include/rp_batch.h)
struct Solution {
    double vel1, duration0, duration1;
    int32_t iters;
    uint32_t status;
};

// Device-side view of one batch: `fields` SoA arrays of `n` elements, field f of the problem at POSITION s at
// base + f * stride + s (stride >= n, an odd multiple of 512 elements: 2-4 KiB aligned fields that do not alias in HBM, rp_batch.cpp).
struct BatchView {
    void *base;            // double* or float*
    size_t stride;         // elements between consecutive fields
    size_t n;              // problems
    int variant;           // 3 or 4
    int dtype;             // 0 = f64, 1 = f32, 2 = f32 state with f64 arithmetic (RP_DTYPE_* of rp_batch.h)
    bool zero_end_vel;     // vel0X == vel2X == 0 for every problem (true after every init the reference has; see Prob in ip_core.h)
    int32_t *iters;        // gated Newton steps taken per problem
    uint32_t *status;      // RP_ST_* bits per problem
    uint32_t *slot_of;     // scheduled order (schedule.hip): problem index -> position in the batch ...
    uint32_t *prob_of;     // ... and position -> problem index; both n words, meaningful while `scheduled`
    StartRecord *records;  // per PROBLEM: the three positions set_problems was given, copied by the scheduling pass; what the
                           // feasible start -- or the fused solve -- of a fresh batch gathers through prob_of.  Null until the
                           // first set_problems
    bool scheduled;        // false: the problems lie in problem order (identical problems of initDefault / initStuck)
    Solution *solution;    // bound by rp_batch_bind_solution (null: none): gated solves write each problem's record there, problem order
    int iters_add;         // ungated steps taken since the last init, added to the iteration counts that leave the batch in records
    unsigned long long *counters;   // 128 words: [0,64) shards of "problems still open after the last gated launch", [64,128) shards of gated steps executed
    uint32_t *lists;       // 2 n + 16 words (null until needed): two position lists + the rounds' counts -- the straggler hand-off of the gated solve
};

struct HostParams {
    double accel_limit, mu_divisor, boundary_fraction, backtrack, armijo;
    int max_backtracks;
    int stall_window;
    int mu_mode;                 // 0 = reference centring, 1 = centring by trial (ip_core.h, newton_step)
    double mu_sigma_try[2];      // the two candidates of mode 1
    int handoff_rounds;          // rp_params.handoff_rounds: 0 = a batch whose order predicts nothing runs the kernel that watches for fixed points, in ONE
                                 // launch; -1 = the plain kernel always; 2..8 = the watching kernel in that many rounds
    int handoff_lanes;           // rp_params.handoff_lanes
};

inline int state_len(int variant) { return variant == 4 ? 12 : 16; }
inline size_t storage_size(int dtype) { return dtype == 0 ? 8 : 4; }      // bytes per state element in HBM
inline int num_constraints(int variant) { return variant == 4 ? 4 : 8; }

// k ungated Newton steps per problem, one launch.
hipError_t launch_steps(const BatchView &b, const HostParams &hp, int k, hipStream_t stream);
// k ungated steps with the per-problem halving totals of both line-search loops (diagnostic twin of launch_steps)
hipError_t launch_steps_counted(const BatchView &b, const HostParams &hp, int k, uint32_t *d_nfeas, uint32_t *d_nresid, hipStream_t stream);
// up to k gated steps per problem (k = max_iter gives the fused solve); zeroes counters[0] first.
hipError_t launch_solve(const BatchView &b, const HostParams &hp, int k, double gap_tol, int max_iter, hipStream_t stream);
// the fused solve (every problem to its gate in one launch).  from_start: the batch holds only its positions (just
// scheduled, schedule.hip) and every problem begins at its feasible start, formed in registers (reference mode, no stall
// detector, zero end velocities only)
hipError_t launch_solve_fused(const BatchView &b, const HostParams &hp, double gap_tol, int max_iter, bool from_start, hipStream_t stream);
// the same for states the batch's order says nothing about (k_solve_chunks<ROUNDS>): a problem whose step leaves its state bit for bit
// unchanged -- a start outside the feasible set -- takes its remaining budget as read (exact), and with rounds > 1 (b.lists must exist) the
// solve runs in ROUNDS: the first launch walks the whole batch and every wave hands its last `lanes` stragglers off -- leaves them open
// and appends their positions to a list -- once they have stepped alone for more than `patience` steps; each further launch walks the
// previous one's list, densely packed, the last one to the end.  Same per-problem arithmetic: same results.
hipError_t launch_solve_rounds(const BatchView &b, const HostParams &hp, double gap_tol, int max_iter, int rounds, int lanes, int patience, hipStream_t stream);
// max ||r||^2, max gap, #converged, gated steps (+ host_steps) -> d_out4 (device); d_partials has 4 * 1024 doubles.
hipError_t launch_reduce(const BatchView &b, const HostParams &hp, double host_steps, double *d_partials,
                         double *d_out4, hipStream_t stream);

// every problem's 32-byte solution record in problem order (walks positions, scatters whole sectors)
hipError_t launch_solution(const BatchView &b, Solution *d_out, hipStream_t stream);
// d(vel1, duration0, duration1) / d(pos0, pos1, pos2) transposed, applied to upstream gradients (null: zeros), problem order in and
// out, at the batch's current state (sensitivity.hip; F3, double storage only)
hipError_t launch_solution_vjp(const BatchView &b, const HostParams &hp, const double *d_g_vel1, const double *d_g_dur0,
                               const double *d_g_dur1, double *d_pos0_bar, double *d_pos1_bar, double *d_pos2_bar, hipStream_t stream);
// d(vel1, duration0, duration1) / d(pos0, pos1, pos2) applied to position tangents (null: zeros), and the whole 3 x 3 Jacobian
// (9 doubles per problem, row-major), problem order in and out, at the batch's current state (sensitivity.hip; F3, double storage only)
hipError_t launch_solution_jvp(const BatchView &b, const HostParams &hp, const double *d_t_pos0, const double *d_t_pos1,
                               const double *d_t_pos2, double *d_t_vel1, double *d_t_dur0, double *d_t_dur1, hipStream_t stream);
hipError_t launch_solution_jacobian(const BatchView &b, const HostParams &hp, double *d_jac, hipStream_t stream);
// d^2(vel1, duration0, duration1) / d(pos0, pos1, pos2)^2 (27 doubles per problem) and, unless d_jac is null, the Jacobian from the
// same first-order solves, problem order, at the batch's current state (sensitivity.hip; F3, double storage only)
hipError_t launch_solution_hessian(const BatchView &b, const HostParams &hp, double *d_jac, double *d_hess, hipStream_t stream);
// the first derivatives in all five boundary inputs (pos0, pos1, pos2, vel0, vel2): VJP, JVP (null tangents / gradients: zeros) and
// the 3 x 5 Jacobian (15 doubles per problem, row-major), problem order, at the batch's current state (sensitivity.hip, the k_endvel_* kernels; F3,
// double storage only)
hipError_t launch_solution_vjp_vel(const BatchView &b, const HostParams &hp, const double *d_g_vel1, const double *d_g_dur0,
                                   const double *d_g_dur1, double *d_pos0_bar, double *d_pos1_bar, double *d_pos2_bar,
                                   double *d_vel0_bar, double *d_vel2_bar, hipStream_t stream);
hipError_t launch_solution_jvp_vel(const BatchView &b, const HostParams &hp, const double *d_t_pos0, const double *d_t_pos1,
                                   const double *d_t_pos2, const double *d_t_vel0, const double *d_t_vel2, double *d_t_vel1,
                                   double *d_t_dur0, double *d_t_dur1, hipStream_t stream);
hipError_t launch_solution_jacobian_vel(const BatchView &b, const HostParams &hp, double *d_jac, hipStream_t stream);

// state movement / initialisation
hipError_t launch_aos_to_soa(const BatchView &b, const double *d_aos, hipStream_t stream);
hipError_t launch_soa_to_aos(const BatchView &b, double *d_aos, hipStream_t stream);
// the feasible start of the positions in the batch's constant fields (rp_batch_restart; the start rule: start_duration, ip_core.h).
// vel: of the positions AND end velocities there, which stay (t_i grows by 8 |vel_end| / L); otherwise the end velocities are zeroed
hipError_t launch_restart(const BatchView &b, const HostParams &hp, bool vel, hipStream_t stream);
// the same from b.records through b.prob_of (a batch that has just been scheduled): positions into the constant fields, the
// feasible start, cleared progress words -- everything k_solve_chunks<START> forms in registers, written out.  vel
// (rp_batch_set_problems_vel_device; b.scheduled): the end velocities are gathered from d_vel0 / d_vel2 (problem order; null: zeros)
// through b.prob_of into their fields; otherwise those fields are zeroed and the two arrays are not looked at
hipError_t launch_start_from_records(const BatchView &b, const HostParams &hp, const double *d_vel0, const double *d_vel2, bool vel, hipStream_t stream);
hipError_t launch_init_const(const BatchView &b, const double *host_state /* state_len values */, hipStream_t stream);
hipError_t launch_nudge(const BatchView &b, int field, double delta, hipStream_t stream);
hipError_t launch_clear_progress(const BatchView &b, hipStream_t stream);
// compute the scheduled order (slot_of / prob_of; schedule.hip) from positions given as three strided double arrays in problem
// order, zero the batch's progress counters and -- write_positions -- copy every problem's three positions into b.records;
// d_scratch: schedule_scratch_bytes(n) bytes of device memory
hipError_t schedule_scratch_bytes(size_t n, size_t *bytes);
// one_wave_blocks: the form of the three kernels whose blocks are single waves (slower alone, able to run beside a solve: what
// rp_pipeline uses); the order is the same either way
hipError_t launch_schedule(const BatchView &b, const double *d_pos0, const double *d_pos1, const double *d_pos2, size_t pstride,
                           bool write_positions, void *d_scratch, size_t scratch_bytes, hipStream_t stream, bool one_wave_blocks = false);
// d_dst[problem] = d_src[position of that problem] for per-problem words kept in batch order (requires b.scheduled)
hipError_t launch_gather_u32(const BatchView &b, const uint32_t *d_src, uint32_t *d_dst, hipStream_t stream);

// the rows either side of the hot path
hipError_t launch_move_toward_feasibility(const BatchView &b, const HostParams &hp, hipStream_t stream);
hipError_t launch_sample(const BatchView &b, double *d_pos66, double *d_acc4, hipStream_t stream);
// the same for a whole scheduled batch with zero end velocities whose b.records still hold its positions: through problem-order
// records (solution records written into d_solution_scratch, n of them, first) instead of the gather through slot_of
hipError_t launch_sample_from_records(const BatchView &b, Solution *d_solution_scratch, double *d_pos66, double *d_acc4, hipStream_t stream);

// the same for problems [first, first + count), plus printState's constraint table (1 + 14 m doubles per problem)
hipError_t launch_soa_to_aos_range(const BatchView &b, size_t first, size_t count, double *d_aos, hipStream_t stream);
hipError_t launch_sample_range(const BatchView &b, size_t first, size_t count, double *d_pos66, double *d_acc4, hipStream_t stream);
hipError_t launch_constraint_table(const BatchView &b, const HostParams &hp, size_t first, size_t count, double *d_rows, hipStream_t stream);


// a spline evaluated at the caller's times, and the evaluation's first derivatives (trajectory.hip, where the plot data above live too).  Tables of eight pointers are
// (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1), n doubles each in problem order; d_tau and everything per query
// n x k doubles, row-major, 16-byte aligned; k < 2^31.  Null pointers as include/rp_batch.h says.
hipError_t launch_trajectory_eval(size_t n, size_t k, const double *const d_spline[8], const double *d_tau, double *d_pos, double *d_vel,
                                  double *d_acc, hipStream_t stream);
hipError_t launch_trajectory_vjp(size_t n, size_t k, const double *const d_spline[8], const double *d_tau, const double *d_g_pos,
                                 const double *d_g_vel, const double *d_g_acc, double *const d_spline_bar[8], double *d_tau_bar, hipStream_t stream);
hipError_t launch_trajectory_jvp(size_t n, size_t k, const double *const d_spline[8], const double *d_tau, const double *const d_spline_dot[8],
                                 const double *d_tau_dot, double *d_pos_dot, double *d_vel_dot, double *d_acc_dot, hipStream_t stream);
// the same evaluation of the batch's current state, problem order, every variant and dtype (launch_sample_range's loader: spline_core.h, FromBatch)
hipError_t launch_trajectory_hvp(size_t n, size_t k, const double *const d_spline[8], const double *d_tau, const double *d_g_pos,
                                 const double *d_g_vel, const double *d_g_acc, const double *const d_spline_dot[8], const double *d_tau_dot,
                                 double *const d_spline_bar_dot[8], double *d_tau_bar_dot, hipStream_t stream);
hipError_t launch_trajectory_batch(const BatchView &b, const double *d_tau, size_t k, double *d_pos, double *d_vel, double *d_acc, hipStream_t stream);
// the first time in [0, duration0 + duration1] at which the spline is at each level (n x k), and the velocity there (null: not wanted);
// stateless and of the batch's current state
hipError_t launch_crossing(size_t n, size_t k, const double *const d_spline[8], const double *d_level, double *d_time, double *d_vel, hipStream_t stream);
hipError_t launch_crossing_batch(const BatchView &b, const double *d_level, size_t k, double *d_time, double *d_vel, hipStream_t stream);
// the extreme position and velocity over the windows [lo, hi] (n x k each; null: -inf / +inf) clamped to [0, duration0 + duration1], and a
// time at which each is attained: tables of four in the order (pos_min, pos_max, vel_min, vel_max), a null entry not wanted
hipError_t launch_extrema(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi, double *const d_value[4],
                          double *const d_time[4], hipStream_t stream);
hipError_t launch_extrema_batch(const BatchView &b, const double *d_lo, const double *d_hi, size_t k, double *const d_value[4],
                                double *const d_time[4], hipStream_t stream);
// the integrals of pos, |vel|, vel^2 and acc^2 over each window (d_value: pos_int, distance, vel_sq, acc_sq), and their first derivatives
hipError_t launch_integrals(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi, double *const d_value[4],
                            hipStream_t stream);
hipError_t launch_integrals_batch(const BatchView &b, const double *d_lo, const double *d_hi, size_t k, double *const d_value[4], hipStream_t stream);
hipError_t launch_integrals_vjp(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi, const double *const d_g[4],
                                double *const d_spline_bar[8], double *d_lo_bar, double *d_hi_bar, hipStream_t stream);
hipError_t launch_integrals_jvp(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi,
                                const double *const d_spline_dot[8], const double *d_lo_dot, const double *d_hi_dot, double *const d_value_dot[4],
                                hipStream_t stream);
// the derivative of launch_integrals_vjp's ten outputs along a direction on the spline and on the window's ends, d_g held fixed
hipError_t launch_integrals_hvp(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi, const double *const d_g[4],
                                const double *const d_spline_dot[8], const double *d_lo_dot, const double *d_hi_dot,
                                double *const d_spline_bar_dot[8], double *d_lo_bar_dot, double *d_hi_bar_dot, hipStream_t stream);
// the extreme gap pos_A(t) - pos_B(t - delay) between two splines over the windows [lo, hi] clamped to their common time domain (lo, hi,
// delay n x k each; null: -inf / +inf / 0), and a time at which each is attained: tables of two in the order (gap_min, gap_max)
hipError_t launch_gap(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                      const double *d_hi, const double *d_delay, double *const d_value[2], double *const d_time[2], hipStream_t stream);
// the integrals of D, D^2 and D'^2 with D(t) = pos_A(t) - pos_B(t - delay) over the same windows: a table of three in the order (gap_int,
// gap_sq, relvel_sq); their reverse rule (d_g: the three upstream gradients, null: zeros; one launch per spline) and forward rule
hipError_t launch_tracking(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                           const double *d_hi, const double *d_delay, double *const d_value[3], hipStream_t stream);
hipError_t launch_tracking_vjp(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                               const double *d_hi, const double *d_delay, const double *const d_g[3], double *const d_spline_a_bar[8],
                               double *const d_spline_b_bar[8], double *d_lo_bar, double *d_hi_bar, double *d_delay_bar, hipStream_t stream);
hipError_t launch_tracking_jvp(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                               const double *d_hi, const double *d_delay, const double *const d_spline_a_dot[8],
                               const double *const d_spline_b_dot[8], const double *d_lo_dot, const double *d_hi_dot, const double *d_delay_dot,
                               double *const d_value_dot[3], hipStream_t stream);
// the derivative of launch_tracking_vjp's nineteen outputs along a direction on both splines and on lo, hi, delay, d_g held fixed
hipError_t launch_tracking_hvp(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                               const double *d_hi, const double *d_delay, const double *const d_g[3], const double *const d_spline_a_dot[8],
                               const double *const d_spline_b_dot[8], const double *d_lo_dot, const double *d_hi_dot, const double *d_delay_dot,
                               double *const d_spline_a_bar_dot[8], double *const d_spline_b_bar_dot[8], double *d_lo_bar_dot,
                               double *d_hi_bar_dot, double *d_delay_bar_dot, hipStream_t stream);
// the first time in the same windows at which D reaches a level (d_level n x k; null: 0), NaN where it does not, and D' there (null: not wanted)
hipError_t launch_meeting(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_level,
                          const double *d_lo, const double *d_hi, const double *d_delay, double *d_time, double *d_relvel, hipStream_t stream);
// the least squared distance of two vehicles of d axes (1..3) over the same windows and when it is attained: the tables hold 8 d pointers,
// axis-major (either output null: not wanted)
hipError_t launch_separation(size_t n, size_t k, int d, const double *const *d_spline_a, const double *const *d_spline_b, const double *d_lo,
                             const double *d_hi, const double *d_delay, double *d_value, double *d_time, hipStream_t stream);
// the first time in the same windows at which that squared distance reaches a level (d_level_sq n x k), NaN where it does not, and its rate
// of change there (null: not wanted)
hipError_t launch_contact(size_t n, size_t k, int d, const double *const *d_spline_a, const double *const *d_spline_b, const double *d_level_sq,
                          const double *d_lo, const double *d_hi, const double *d_delay, double *d_time, double *d_rate, hipStream_t stream);
// that least squared distance and its time for every pair (i, j), i < j, of n scenes of m vehicles (2..256) on one clock: d_fleet holds 8 d
// pointers, axis-major, to arrays of n m values (vehicle v of scene s at s m + v); d_lo, d_hi n x k (null: -inf, +inf); the outputs
// n x m (m - 1) / 2 x k, pairs in lexicographic order (either null: not wanted)
hipError_t launch_fleet_separation(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_lo, const double *d_hi,
                                   double *d_value, double *d_time, hipStream_t stream);
// the first time a pair's squared distance reaches a level, for every pair of such a fleet: d_level_sq n x k (level_per_pair 0: one level for
// all pairs of a scene) or n x m (m - 1) / 2 x k (1); d_time required, d_rate may be null; both n x m (m - 1) / 2 x k
hipError_t launch_fleet_contact(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_level_sq, int level_per_pair,
                                const double *d_lo, const double *d_hi, double *d_time, double *d_rate, hipStream_t stream);
// the same two queries for every vehicle of fleet A (m_a of them, 1..32768) against every vehicle of fleet B (m_b) of n scenes on one clock
// (DESIGN.md section 34): d_fleet_a holds 8 d pointers to arrays of n m_a values, d_fleet_b to n m_b; the windows, the level's two layouts
// and the optional outputs as in the two fleet launches; the outputs n x m_a m_b x k, pair (i, j) at i m_b + j
hipError_t launch_cross_separation(size_t n, size_t m_a, size_t m_b, size_t k, int d, const double *const *d_fleet_a, const double *const *d_fleet_b,
                                   const double *d_lo, const double *d_hi, double *d_value, double *d_time, hipStream_t stream);
hipError_t launch_cross_contact(size_t n, size_t m_a, size_t m_b, size_t k, int d, const double *const *d_fleet_a, const double *const *d_fleet_b,
                                const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi, double *d_time,
                                double *d_rate, hipStream_t stream);
// the two fleet queries with a start time per vehicle, d_start n x m (required) on the scene's clock, on which d_lo, d_hi and d_time are;
// d_time_local is the same time on the clock of the pair's first vehicle (any output may be null, not all)
hipError_t launch_fleet_separation_staggered(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_start,
                                             const double *d_lo, const double *d_hi, double *d_value, double *d_time, double *d_time_local,
                                             hipStream_t stream);
hipError_t launch_fleet_contact_staggered(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_start,
                                          const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi, double *d_time,
                                          double *d_time_local, double *d_rate, hipStream_t stream);
// the fleet's position boxes over the scenes' windows: d_min, d_max d pointers each to n x m x k (null table or entry: not wanted),
// d_slack d pointers to n x m (null table: not wanted).  d_start (n x m) given: the window of vehicle v on its own clock (DESIGN.md
// section 31), and d_total and d_speed, d pointers to n x m each, next to the slacks; d_start null: one clock, and neither is looked at
hipError_t launch_fleet_reach(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_start, const double *d_lo,
                              const double *d_hi, double *const *d_min, double *const *d_max, double *const *d_slack, double *const *d_total,
                              double *const *d_speed, hipStream_t stream);
// launch_fleet_contact (d_start null; section 30) or launch_fleet_contact_staggered (d_start given; section 31) with the broad phase in
// front (section 32): the bytes of workspace it needs (0: n x pairs does not fit 32 bits), and the launch -- boxes, sieve, list and the
// search over the list: on one clock where d_time is given (d_time_local is not looked at), with starts where any of the three outputs is.
// Otherwise: the broad phase alone.  d_kept (n x pairs bytes), d_list (n x pairs uint32) and d_count (one uint32) are copies for the
// caller (null: none).
size_t fleet_cull_workspace_bytes(size_t n, size_t m, size_t k, int d, bool staggered);
hipError_t launch_fleet_contact_culled(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_start,
                                       const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi, double *d_time,
                                       double *d_time_local, double *d_rate, void *d_workspace, unsigned char *d_kept, uint32_t *d_list,
                                       uint32_t *d_count, hipStream_t stream);

}  // namespace rp
