// sensitivity.hip -- vector-Jacobian product of an F3 solution with respect to the positions (rp_batch_solution_vjp), gfx950.
//
// For the state z = (x, lam), x = (vel1, duration0, duration1), the reference's residual r(z; theta, p) (onedpath_ip.cpp:753-783,
// p held fixed) and M = dr/dz, the Newton matrix moveInteriorPoint assembles (onedpath_ip.cpp:814-861):
//     M^T w = [g; 0_8],    theta_bar = -w^T dr/dtheta,    theta = (pos0, pos1, pos2)
// -- the implicit-function derivative of the central-path point at this p.  M^T = [[W, G^T Lam], [G, C]]
// condenses as the forward system does:
//     w_lam = -C^-1 G w_x,    K w_x = g,    K = W - G^T Lam C^-1 G = W + S_j D_j h_j h_j^T
// with h_j = grad a_j and D_j = lam_p / (-c_p) + lam_m / (-c_m) of the constraint pair on acceleration j; K is solved by Gaussian
// elimination with partial pivoting, every quotient an IEEE division.  The theta-derivative then needs only
//     s_j = lam_p w_lam_p - lam_m w_lam_m = D_j h_j . w_x     (the multiplier-weighted dual step of pair j)
// because r depends on theta only through dX0 = pos1 - pos0, dX1 = pos2 - pos1, affinely:
//     d a / d dX = +-6 / t^2,   d (d a / d t) / d dX = -+12 / t^3,   d (d a / d v) / d dX = 0.
// Why this form is accurate although D_j reaches ~1e8 relative on active rows: on the states a solve returns, lam_i c_i ~ -p for
// every constraint, so D_j is either huge (active: lam^2 / p) or tiny (inactive: p / c^2) -- no pair sits in between.  The huge
// part of K is H_A^T D_A H_A, and the product that matters, s_A = D_A H_A K^-1 g, has the large factors cancel analytically
// (s_A -> H_A^-T g): an elimination error of eps relative to K itself reaches s as eps times cond(H_A)-sized factors, not times D.
// Measured against a longdouble elimination of the full 11 x 11 system (tests/test_sensitivity_cpu.py): ~1e-14 normwise on the
// monotone and reference-like distributions, ~1e-11 on the degenerate non-monotone one.
//
// One lane per problem, walking batch positions like k_solution: 16 fields read coalesced, the upstream gradient gathered at
// prob_of[s], theta_bar scattered there -- problem order in and out.
#include "ip_kernels.h"

#include "../../include/rp_batch.h"
#include "ip_core.h"

namespace rp {

namespace {

constexpr int kVjpBlock = 256;

// x = A^-1 b for a 3 x 3 system: Gaussian elimination with partial pivoting.  The row swaps are selects on registers
// (a dynamically indexed row would go to scratch).
__device__ __forceinline__ void solve3_pivoted(double (&A)[3][3], double (&b)[3], double (&x)[3])
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int r = k + 1; r < 3; ++r) {
            const bool sw = __builtin_fabs(A[r][k]) > __builtin_fabs(A[k][k]);
#pragma unroll
            for (int c = k; c < 3; ++c) {
                const double a = A[k][c], o = A[r][c];
                A[k][c] = sw ? o : a;
                A[r][c] = sw ? a : o;
            }
            const double a = b[k], o = b[r];
            b[k] = sw ? o : a;
            b[r] = sw ? a : o;
        }
#pragma unroll
        for (int r = k + 1; r < 3; ++r) {
            const double f = A[r][k] / A[k][k];
#pragma unroll
            for (int c = k + 1; c < 3; ++c) A[r][c] -= f * A[k][c];
            b[r] -= f * b[k];
        }
    }
    x[2] = b[2] / A[2][2];
    x[1] = (b[1] - A[1][2] * x[2]) / A[1][1];
    x[0] = (b[0] - A[0][1] * x[1] - A[0][2] * x[2]) / A[0][0];
}

__global__ void __launch_bounds__(kVjpBlock)
k_solution_vjp(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
               const double *__restrict__ g_vel1, const double *__restrict__ g_dur0, const double *__restrict__ g_dur1,
               double *__restrict__ pos0_bar, double *__restrict__ pos1_bar, double *__restrict__ pos2_bar)
{
    const size_t s = (size_t)blockIdx.x * kVjpBlock + threadIdx.x;
    if (s >= n) return;
    double f[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) f[i] = __builtin_nontemporal_load(base + (size_t)i * stride + s);
    const size_t prob = prob_of ? (size_t)prob_of[s] : s;
    const double g[3] = {g_vel1 ? g_vel1[prob] : 0.0, g_dur0 ? g_dur0[prob] : 0.0, g_dur1 ? g_dur1[prob] : 0.0};

    const double v = f[0], t0 = f[1], t1 = f[2];
    const double *lam = f + 3;
    Prob<double> k;
    k.v0 = f[12];
    k.v2 = f[15];
    k.dx0 = f[13] - f[11];
    k.dx1 = f[14] - f[13];
    Acc<double> e;
    accel_values(k, v, t0, t1, e);
    accel_grads(k, v, e);
    double htt[4], htv[4];
    accel_hess(k, v, e, htt, htv);

    // NaN for the states RP_ST_NONFINITE / RP_ST_INFEASIBLE describe: not finite, or some c_i > 0 (constraintsSatisfied,
    // onedpath_ip.cpp:738-751).  Below gaps of ~1e-12 an active constraint's value is under the rounding of a - L and can come out
    // as exactly 0: |c| is floored at the forward step's c_floor (L eps / 256).  D of that pair is then huge either way, and the
    // result does not depend on it (s_A -> H_A^-T g).
    bool ok = true;
#pragma unroll
    for (int i = 0; i < 16; ++i) ok = ok && finite_(f[i]);
    const double c_floor = limit * 8.673617379884035e-19;
    double D[4], mu[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double cm = c_value<double, 3>(2 * j, e, limit), cp = c_value<double, 3>(2 * j + 1, e, limit);
        const double lm = lam[2 * j], lp = lam[2 * j + 1];
        ok = ok && !(cm > 0.0) && !(cp > 0.0);
        D[j] = lp / max_(-cp, c_floor) + lm / max_(-cm, c_floor);
        mu[j] = lp - lm;      // S lam_i g_i = (lp - lm) grad a_j: the pair's weight in W = S lam_i H_i
    }

    // K = W + S_j D_j h_j h_j^T in (vel1, duration0, duration1); K(t0, t1) = 0 (no constraint touches both durations)
    double gv[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) gv[j] = acc_gv(e, j);
    double K[3][3];
    K[0][0] = D[0] * gv[0] * gv[0] + D[1] * gv[1] * gv[1] + D[2] * gv[2] * gv[2] + D[3] * gv[3] * gv[3];
    K[0][1] = mu[0] * htv[0] + mu[1] * htv[1] + D[0] * gv[0] * e.gt[0] + D[1] * gv[1] * e.gt[1];
    K[0][2] = mu[2] * htv[2] + mu[3] * htv[3] + D[2] * gv[2] * e.gt[2] + D[3] * gv[3] * e.gt[3];
    K[1][1] = mu[0] * htt[0] + mu[1] * htt[1] + D[0] * e.gt[0] * e.gt[0] + D[1] * e.gt[1] * e.gt[1];
    K[2][2] = mu[2] * htt[2] + mu[3] * htt[3] + D[2] * e.gt[2] * e.gt[2] + D[3] * e.gt[3] * e.gt[3];
    K[1][0] = K[0][1];
    K[2][0] = K[0][2];
    K[1][2] = K[2][1] = 0.0;
    double rhs[3] = {g[0], g[1], g[2]}, w[3];
    solve3_pivoted(K, rhs, w);

    double sj[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) sj[j] = D[j] * (gv[j] * w[0] + e.gt[j] * w[1 + (j >> 1)]);
    const double q0 = e.r0 * e.r0, q1 = e.r1 * e.r1;
    const double dx0_bar = -(12.0 * q0 * e.r0 * w[1] * (mu[1] - mu[0]) + 6.0 * q0 * (sj[0] - sj[1]));
    const double dx1_bar = -(12.0 * q1 * e.r1 * w[2] * (mu[3] - mu[2]) + 6.0 * q1 * (sj[2] - sj[3]));
    const double nan = __builtin_nan("");
    pos0_bar[prob] = ok ? -dx0_bar : nan;
    pos1_bar[prob] = ok ? dx0_bar - dx1_bar : nan;
    pos2_bar[prob] = ok ? dx1_bar : nan;
}

}  // namespace

hipError_t launch_solution_vjp(const BatchView &b, const HostParams &hp, const double *d_g_vel1, const double *d_g_dur0,
                               const double *d_g_dur1, double *d_pos0_bar, double *d_pos1_bar, double *d_pos2_bar, hipStream_t stream)
{
    if (b.n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((b.n + kVjpBlock - 1) / kVjpBlock);
    hipLaunchKernelGGL(k_solution_vjp, dim3(blocks), dim3(kVjpBlock), 0, stream, (const double *)b.base, b.stride, b.n,
                       b.scheduled ? (const uint32_t *)b.prob_of : nullptr, hp.accel_limit, d_g_vel1, d_g_dur0, d_g_dur1,
                       d_pos0_bar, d_pos1_bar, d_pos2_bar);
    return hipGetLastError();
}

}  // namespace rp
