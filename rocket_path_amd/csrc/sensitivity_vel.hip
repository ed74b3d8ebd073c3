// sensitivity_vel.hip -- first derivatives of an F3 solution in all five boundary inputs theta = (pos0, pos1, pos2, vel0, vel2),
// gfx950: the vector-Jacobian product (rp_batch_solution_vjp_vel), the Jacobian-vector product (rp_batch_solution_jvp_vel) and the
// per-problem 3 x 5 Jacobian (rp_batch_solution_jacobian_vel).
//
// Same z, r, p, M, condensed double-double K and NaN rule as sensitivity.hip (shared code: sensitivity_core.h); the position parts
// run that file's arithmetic operation for operation.  The end velocities have the shape of the position deltas and enter only their
// own segment's two accelerations, affinely (a_j = 6 sg_j dX / t^2 + w_j / t, w_j = -4 vel0 - 2 v, 2 vel0 + 4 v, -4 v - 2 vel2,
// 2 v + 4 vel2; onedpath_ip.cpp:1025-1028):
//     segment 0:  d a / d vel0 = (-4, +2) / t0,    d (d a / d t0) / d vel0 = (+4, -2) / t0^2
//     segment 1:  d a / d vel2 = (-2, +4) / t1,    d (d a / d t1) / d vel2 = (+2, -4) / t1^2
// and d (d a / d vel1) / d vel_end = 0, so a velocity direction adds to the durations' rows of b_x and to the pairs' alpha_j exactly
// as a dX direction does (sensitivity.hip's opening comment), with these coefficients.  A state with a non-positive duration gets NaN
// besides those sensitivity.hip gives NaN for: with end velocities the reference's backtracking can step over t = 0 (DESIGN.md
// section 12), and there the formula describes no trajectory.
//
// One lane per problem as in sensitivity.hip: 16 fields read coalesced, inputs gathered and results scattered at prob_of[s].
#include "ip_kernels.h"

#include "../../include/rp_batch.h"
#include "ip_core.h"
#include "sensitivity_core.h"

namespace rp {

namespace {

// the formula applies: sensitivity.hip's rule, and both durations positive
__device__ __forceinline__ bool condense_vel(const double (&f)[16], double limit, Condensed &c)
{
    const bool ok = condense(f, limit, c);
    return ok && f[1] > 0.0 && f[2] > 0.0;
}

// The condensed forward right-hand side -b_x - S_j D_j alpha_j h_j of all five tangents: forward_rhs's, with the end-velocity tangents
// (e0, e2) = (vel0_dot, vel2_dot) added to its alpha_j and b_x before the double-double products:
//     alpha_j += (-4 e0, 2 e0) / t0, (-2 e2, 4 e2) / t1,    b_x += (0, (4 mu_0 - 2 mu_1) e0 / t0^2, (2 mu_2 - 4 mu_3) e2 / t1^2).
// With e0 = e2 = 0 the additions are of zeros: forward_rhs's values bit for bit.
__device__ __forceinline__ void forward_rhs5(const Condensed &c, double dd0, double dd1, double e0, double e2, ddv (&rhs)[3])
{
    const Acc<double> &e = c.e;
    const double q0 = e.r0 * e.r0, q1 = e.r1 * e.r1;
    const double al[4] = {6.0 * q0 * dd0 + -4.0 * e.r0 * e0, -(6.0 * q0 * dd0) + 2.0 * e.r0 * e0,
                          6.0 * q1 * dd1 + -2.0 * e.r1 * e2, -(6.0 * q1 * dd1) + 4.0 * e.r1 * e2};
    rhs[0] = dd_neg(dd_add(dd_add(dd_mul_d(c.Dgv[0], al[0]), dd_mul_d(c.Dgv[1], al[1])),
                           dd_add(dd_mul_d(c.Dgv[2], al[2]), dd_mul_d(c.Dgv[3], al[3]))));
    rhs[1] = dd_neg(dd_add(dd_of(12.0 * q0 * e.r0 * dd0 * (c.mu[1] - c.mu[0]) + q0 * e0 * (4.0 * c.mu[0] - 2.0 * c.mu[1])),
                           dd_add(dd_mul_d(c.Dgt[0], al[0]), dd_mul_d(c.Dgt[1], al[1]))));
    rhs[2] = dd_neg(dd_add(dd_of(12.0 * q1 * e.r1 * dd1 * (c.mu[3] - c.mu[2]) + q1 * e2 * (2.0 * c.mu[2] - 4.0 * c.mu[3])),
                           dd_add(dd_mul_d(c.Dgt[2], al[2]), dd_mul_d(c.Dgt[3], al[3]))));
}

// solve3_dd split in two: lu3_dd runs its elimination on K once, keeping the row swaps and the multipliers f (in A's lower part), and
// lu3_dd_solve applies them to one right-hand side -- the same swaps, updates and back substitution, operation for operation, as
// solve3_dd gives that right-hand side (its updates of B read only B, the swaps and f), so the results are solve3_dd's bit for bit.  For
// the Jacobian's four directions: one elimination of K, and one right-hand side live at a time.
__device__ __forceinline__ void lu3_dd(ddv (&A)[3][3], bool (&sw)[3])
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int r = k + 1; r < 3; ++r) {
            const bool w = __builtin_fabs(A[r][k].hi) > __builtin_fabs(A[k][k].hi);
            sw[k + r - 1] = w;      // (k, r) = (0, 1), (0, 2), (1, 2) -> 0, 1, 2
#pragma unroll
            for (int c = k; c < 3; ++c) {
                const ddv a = A[k][c], o = A[r][c];
                A[k][c] = w ? o : a;
                A[r][c] = w ? a : o;
            }
        }
#pragma unroll
        for (int r = k + 1; r < 3; ++r) {
            const ddv f = dd_div(A[r][k], A[k][k]);
#pragma unroll
            for (int c = k + 1; c < 3; ++c) A[r][c] = dd_sub(A[r][c], dd_mul(f, A[k][c]));
            A[r][k] = f;
        }
    }
}

__device__ __forceinline__ void lu3_dd_solve(const ddv (&A)[3][3], const bool (&sw)[3], ddv (&B)[3], ddv (&X)[3])
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int r = k + 1; r < 3; ++r) {
            const bool w = sw[k + r - 1];
            const ddv a = B[k], o = B[r];
            B[k] = w ? o : a;
            B[r] = w ? a : o;
        }
#pragma unroll
        for (int r = k + 1; r < 3; ++r) B[r] = dd_sub(B[r], dd_mul(A[r][k], B[k]));
    }
#pragma unroll
    for (int k = 2; k >= 0; --k) {
        ddv acc = B[k];
#pragma unroll
        for (int c = k + 1; c < 3; ++c) acc = dd_sub(acc, dd_mul(A[k][c], X[c]));
        X[k] = dd_div(acc, A[k][k]);
    }
}

__global__ void __launch_bounds__(kVjpBlock)
k_endvel_vjp(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
             const double *__restrict__ g_vel1, const double *__restrict__ g_dur0, const double *__restrict__ g_dur1,
             double *__restrict__ pos0_bar, double *__restrict__ pos1_bar, double *__restrict__ pos2_bar,
             double *__restrict__ vel0_bar, double *__restrict__ vel2_bar)
{
    const size_t s = (size_t)blockIdx.x * kVjpBlock + threadIdx.x;
    if (s >= n) return;
    double f[16];
    load_fields(base, stride, s, f);
    const size_t prob = prob_of ? (size_t)prob_of[s] : s;

    Condensed c;
    const bool ok = condense_vel(f, limit, c);
    condense_K(c);
    ddv rhs[1][3] = {{dd_of(g_vel1 ? g_vel1[prob] : 0.0), dd_of(g_dur0 ? g_dur0[prob] : 0.0), dd_of(g_dur1 ? g_dur1[prob] : 0.0)}};
    ddv w[1][3];
    solve3_dd<1>(c.K, rhs, w);

    double sj[4];      // k_solution_vjp's s_j
#pragma unroll
    for (int j = 0; j < 4; ++j) sj[j] = dd_add(dd_mul(c.Dgv[j], w[0][0]), dd_mul(c.Dgt[j], w[0][1 + (j >> 1)])).hi;
    const Acc<double> &e = c.e;
    const double q0 = e.r0 * e.r0, q1 = e.r1 * e.r1;
    const double dx0_bar = -(12.0 * q0 * e.r0 * w[0][1].hi * (c.mu[1] - c.mu[0]) + 6.0 * q0 * (sj[0] - sj[1]));
    const double dx1_bar = -(12.0 * q1 * e.r1 * w[0][2].hi * (c.mu[3] - c.mu[2]) + 6.0 * q1 * (sj[2] - sj[3]));
    const double v0_bar = -(q0 * w[0][1].hi * (4.0 * c.mu[0] - 2.0 * c.mu[1]) + e.r0 * (2.0 * sj[1] - 4.0 * sj[0]));
    const double v2_bar = -(q1 * w[0][2].hi * (2.0 * c.mu[2] - 4.0 * c.mu[3]) + e.r1 * (4.0 * sj[3] - 2.0 * sj[2]));
    const double nan = __builtin_nan("");
    pos0_bar[prob] = ok ? -dx0_bar : nan;
    pos1_bar[prob] = ok ? dx0_bar - dx1_bar : nan;
    pos2_bar[prob] = ok ? dx1_bar : nan;
    vel0_bar[prob] = ok ? v0_bar : nan;
    vel2_bar[prob] = ok ? v2_bar : nan;
}

__global__ void __launch_bounds__(kVjpBlock)
k_endvel_jvp(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
             const double *__restrict__ t_pos0, const double *__restrict__ t_pos1, const double *__restrict__ t_pos2,
             const double *__restrict__ t_vel0, const double *__restrict__ t_vel2,
             double *__restrict__ t_vel1, double *__restrict__ t_dur0, double *__restrict__ t_dur1)
{
    const size_t s = (size_t)blockIdx.x * kVjpBlock + threadIdx.x;
    if (s >= n) return;
    double f[16];
    load_fields(base, stride, s, f);
    const size_t prob = prob_of ? (size_t)prob_of[s] : s;
    const double tp0 = t_pos0 ? t_pos0[prob] : 0.0, tp1 = t_pos1 ? t_pos1[prob] : 0.0, tp2 = t_pos2 ? t_pos2[prob] : 0.0;
    const double tv0 = t_vel0 ? t_vel0[prob] : 0.0, tv2 = t_vel2 ? t_vel2[prob] : 0.0;

    Condensed c;
    const bool ok = condense_vel(f, limit, c);
    condense_K(c);
    ddv rhs[1][3], xd[1][3];
    forward_rhs5(c, tp1 - tp0, tp2 - tp1, tv0, tv2, rhs[0]);      // zero velocity tangents: k_solution_jvp's right-hand side
    solve3_dd<1>(c.K, rhs, xd);
    const double nan = __builtin_nan("");
    t_vel1[prob] = ok ? xd[0][0].hi : nan;
    t_dur0[prob] = ok ? xd[0][1].hi : nan;
    t_dur1[prob] = ok ? xd[0][2].hi : nan;
}

// J[a][b] = d x_a / d theta_b, b over (pos0, pos1, pos2, vel0, vel2), at jac[15 i + 5 a + b].  The four right-hand sides (dX0, dX1,
// vel0, vel2) are formed first, so that D_j h_j and mu_j are dead before the elimination; K is eliminated once (lu3_dd) and applied to
// them one at a time.  The position columns are k_solution_jacobian's arithmetic.  128 VGPRs (one solve3_dd on all four, or two pairs
// on copies of K: 134-140).
__global__ void __launch_bounds__(kVjpBlock)
k_endvel_jacobian(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
                  double *__restrict__ jac)
{
    const size_t s = (size_t)blockIdx.x * kVjpBlock + threadIdx.x;
    if (s >= n) return;
    double f[16];
    load_fields(base, stride, s, f);
    const size_t prob = prob_of ? (size_t)prob_of[s] : s;

    Condensed c;
    const bool ok = condense_vel(f, limit, c);
    condense_K(c);
    ddv rhs[4][3];      // directions dX0, dX1, vel0, vel2, formed first: D_j h_j and mu_j are dead before the elimination
    forward_rhs(c, 1.0, 0.0, rhs[0]);
    forward_rhs(c, 0.0, 1.0, rhs[1]);
    forward_rhs5(c, 0.0, 0.0, 1.0, 0.0, rhs[2]);
    forward_rhs5(c, 0.0, 0.0, 0.0, 1.0, rhs[3]);
    rhs[2][2] = rhs[3][1] = dd_of(0.0);      // a velocity enters only its own segment's duration row (the kernel cannot know these are 0)
    bool sw[3];
    lu3_dd(c.K, sw);
    const double nan = __builtin_nan("");
    double *out = jac + prob * 15;
    double d0[3];      // dx / d dX0, until dx / d dX1 is known: column pos1 is their difference (dX0 = pos1 - pos0, dX1 = pos2 - pos1)
#pragma unroll
    for (int k = 0; k < 4; ++k) {      // one right-hand side after the other; every column stored as soon as it is known
        ddv X[3];
        lu3_dd_solve(c.K, sw, rhs[k], X);
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const double x = X[a].hi;
            if (k == 0) { d0[a] = x; out[5 * a + 0] = ok ? -x : nan; }
            else if (k == 1) { out[5 * a + 1] = ok ? d0[a] - x : nan; out[5 * a + 2] = ok ? x : nan; }
            else out[5 * a + k + 1] = ok ? x : nan;
        }
    }
}

}  // namespace

hipError_t launch_solution_vjp_vel(const BatchView &b, const HostParams &hp, const double *d_g_vel1, const double *d_g_dur0,
                                   const double *d_g_dur1, double *d_pos0_bar, double *d_pos1_bar, double *d_pos2_bar,
                                   double *d_vel0_bar, double *d_vel2_bar, hipStream_t stream)
{
    if (b.n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((b.n + kVjpBlock - 1) / kVjpBlock);
    hipLaunchKernelGGL(k_endvel_vjp, dim3(blocks), dim3(kVjpBlock), 0, stream, (const double *)b.base, b.stride, b.n,
                       b.scheduled ? (const uint32_t *)b.prob_of : nullptr, hp.accel_limit, d_g_vel1, d_g_dur0, d_g_dur1,
                       d_pos0_bar, d_pos1_bar, d_pos2_bar, d_vel0_bar, d_vel2_bar);
    return hipGetLastError();
}

hipError_t launch_solution_jvp_vel(const BatchView &b, const HostParams &hp, const double *d_t_pos0, const double *d_t_pos1,
                                   const double *d_t_pos2, const double *d_t_vel0, const double *d_t_vel2, double *d_t_vel1,
                                   double *d_t_dur0, double *d_t_dur1, hipStream_t stream)
{
    if (b.n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((b.n + kVjpBlock - 1) / kVjpBlock);
    hipLaunchKernelGGL(k_endvel_jvp, dim3(blocks), dim3(kVjpBlock), 0, stream, (const double *)b.base, b.stride, b.n,
                       b.scheduled ? (const uint32_t *)b.prob_of : nullptr, hp.accel_limit, d_t_pos0, d_t_pos1, d_t_pos2,
                       d_t_vel0, d_t_vel2, d_t_vel1, d_t_dur0, d_t_dur1);
    return hipGetLastError();
}

hipError_t launch_solution_jacobian_vel(const BatchView &b, const HostParams &hp, double *d_jac, hipStream_t stream)
{
    if (b.n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((b.n + kVjpBlock - 1) / kVjpBlock);
    hipLaunchKernelGGL(k_endvel_jacobian, dim3(blocks), dim3(kVjpBlock), 0, stream, (const double *)b.base, b.stride, b.n,
                       b.scheduled ? (const uint32_t *)b.prob_of : nullptr, hp.accel_limit, d_jac);
    return hipGetLastError();
}

}  // namespace rp
