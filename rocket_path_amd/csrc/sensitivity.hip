// sensitivity.hip -- derivatives of an F3 solution, gfx950.  With respect to the positions: the vector-Jacobian product
// (rp_batch_solution_vjp), the Jacobian-vector product (rp_batch_solution_jvp), the per-problem 3 x 3 Jacobian
// (rp_batch_solution_jacobian) and the per-problem 3 x 3 x 3 Hessian (rp_batch_solution_hessian, see k_solution_hessian).  First
// derivatives in all five boundary inputs theta = (pos0, pos1, pos2, vel0, vel2): the vector-Jacobian product
// (rp_batch_solution_vjp_vel), the Jacobian-vector product (rp_batch_solution_jvp_vel) and the per-problem 3 x 5 Jacobian
// (rp_batch_solution_jacobian_vel).  Each first derivative is stated once, as a body templated on `Vel`; its two kernels
// (k_solution_*, k_endvel_*) instantiate it, and what exists only with end velocities sits behind `if constexpr (Vel)`.
//
// For the state z = (x, lam), x = (vel1, duration0, duration1), the reference's residual r(z; theta, p) (onedpath_ip.cpp:753-783,
// p held fixed) and M = dr/dz, the Newton matrix moveInteriorPoint assembles (onedpath_ip.cpp:814-861):
//     reverse:  M^T w = [g; 0_8],    theta_bar = -w^T dr/dtheta,    theta = (pos0, pos1, pos2)
//     forward:  M z_dot = -(dr/dtheta) theta_dot,    x_dot = the x part of z_dot
// -- the implicit-function derivative of the central-path point at this p.  M = [[W, G^T], [Lam G, C]]
// condenses as the Newton step does, in both directions with the same symmetric matrix:
//     w_lam = -C^-1 G w_x,    K w_x = g,    K = W - G^T Lam C^-1 G = W + S_j D_j h_j h_j^T
// with h_j = grad a_j and D_j = lam_p / (-c_p) + lam_m / (-c_m) of the constraint pair on acceleration j; K is formed and solved by
// Gaussian elimination with partial pivoting in double-double (see below).  The theta-derivative then needs only
//     s_j = lam_p w_lam_p - lam_m w_lam_m = D_j h_j . w_x     (the multiplier-weighted dual step of pair j)
// because r depends on theta only through dX0 = pos1 - pos0, dX1 = pos2 - pos1, affinely:
//     d a / d dX = +-6 / t^2,   d (d a / d t) / d dX = -+12 / t^3,   d (d a / d v) / d dX = 0.
// Forward, with b = (dr/dtheta) theta_dot: the complementarity rows give lam_dot_i = -(b_i + lam_i grad c_i . x_dot) / c_i, and
//     K x_dot = -b_x + S_i grad c_i b_i / c_i = -b_x - S_j D_j alpha_j h_j
// where alpha_j = (d a_j / d dX) dX_dot is the tangent of acceleration j (b_i = +-lam_i alpha_j on the pair, so a pair's two terms
// sum to D_j: the large factors appear once, in the VJP's D_j h_j shape) and b_x = S_j mu_j beta_j, mu_j = lam_p - lam_m,
// beta_j = (d (d a_j / d t) / d dX) dX_dot, sits in the duration rows only.
// Why double-double: D_j reaches lam^2 / p on an active pair (~1e8 at gap 1e-8, ~1e12 at 1e-13, ~1e17 where |c| is floored).  Where
// the active rows H_A leave a null space (two active constraints, some with three), the solution's component in it is set by W
// alone, which sits that far below D_A h h^T in K: a K rounded to float64 loses it (errors up to 1e2 relative).  With every product
// D_j h_j exact and K, the forward right-hand side and the elimination in ~106 bits, the result is the exact solution of the
// condensed system for the float64 inputs W, h_j, D_j -- that is, of the well-conditioned system [[W, H^T], [H, -diag(1 / D)]]
// (eliminating its last four unknowns gives K), whose inputs' rounding moves the answer by its own condition number times eps.
// That 7 x 7 system solved in float64 would do the same but does not fit the register budget.  Measured
// against a longdouble elimination of the full 11 x 11 system (tests/test_sensitivity_edges_cpu.py and the first-order CPU tests):
// ~1e-14 normwise on the generators' problems, <= 5e-12 with non-zero end velocities.
//
// With end velocities (Vel): same z, r, p, M, condensed double-double K and NaN rule; the position parts run the arithmetic above
// operation for operation.  The end velocities have the shape of the position deltas and enter only their
// own segment's two accelerations, affinely (a_j = 6 sg_j dX / t^2 + w_j / t, w_j = -4 vel0 - 2 v, 2 vel0 + 4 v, -4 v - 2 vel2,
// 2 v + 4 vel2; onedpath_ip.cpp:1025-1028):
//     segment 0:  d a / d vel0 = (-4, +2) / t0,    d (d a / d t0) / d vel0 = (+4, -2) / t0^2
//     segment 1:  d a / d vel2 = (-2, +4) / t1,    d (d a / d t1) / d vel2 = (+2, -4) / t1^2
// and d (d a / d vel1) / d vel_end = 0, so a velocity direction adds to the durations' rows of b_x and to the pairs' alpha_j exactly
// as a dX direction does, with these coefficients.  A state with a non-positive duration gets NaN besides those the position
// derivatives give NaN for: with end velocities the reference's backtracking can step over t = 0, and there
// the formula describes no trajectory.
//
// One lane per problem, walking batch positions like k_solution (load_lane): 16 fields read coalesced, the per-problem inputs
// gathered at prob_of[s], the results scattered there -- problem order in and out.
#include "ip_kernels.h"

#include "../../include/rp_batch.h"
#include "ip_core.h"
#include "sensitivity_core.h"

namespace rp {

namespace {

// theta_bar = J^T g.  Vel: also vel0_bar and vel2_bar (otherwise not read).
template <bool Vel>
__device__ __forceinline__ void solution_vjp(const double *base, size_t stride, size_t n, const uint32_t *prob_of, double limit,
                                             const double *g_vel1, const double *g_dur0, const double *g_dur1, double *pos0_bar,
                                             double *pos1_bar, double *pos2_bar, double *vel0_bar, double *vel2_bar)
{
    double f[16];
    size_t prob;
    if (!load_lane(base, stride, n, prob_of, f, prob)) return;

    Condensed c;
    const bool ok = condense_with_K<Vel>(f, limit, c);
    ddv rhs[1][3] = {{dd_of(g_vel1 ? g_vel1[prob] : 0.0), dd_of(g_dur0 ? g_dur0[prob] : 0.0), dd_of(g_dur1 ? g_dur1[prob] : 0.0)}};
    ddv w[1][3];
    solve3_dd<1>(c.K, rhs, w);

    double sj[4];      // s_j = D_j h_j . w: the pair's multiplier-weighted dual step, from the exact D_j h_j and the double-double w
#pragma unroll
    for (int j = 0; j < 4; ++j) sj[j] = dd_add(dd_mul(c.Dgv[j], w[0][0]), dd_mul(c.Dgt[j], w[0][1 + (j >> 1)])).hi;
    const Acc<double> &e = c.e;
    const double q0 = e.r0 * e.r0, q1 = e.r1 * e.r1;
    const double dx0_bar = -(12.0 * q0 * e.r0 * w[0][1].hi * (c.mu[1] - c.mu[0]) + 6.0 * q0 * (sj[0] - sj[1]));
    const double dx1_bar = -(12.0 * q1 * e.r1 * w[0][2].hi * (c.mu[3] - c.mu[2]) + 6.0 * q1 * (sj[2] - sj[3]));
    const double nan = __builtin_nan("");
    double v0_bar, v2_bar;
    if constexpr (Vel) {      // formed before the position outputs are stored, as k_endvel_vjp always has
        v0_bar = -(q0 * w[0][1].hi * (4.0 * c.mu[0] - 2.0 * c.mu[1]) + e.r0 * (2.0 * sj[1] - 4.0 * sj[0]));
        v2_bar = -(q1 * w[0][2].hi * (2.0 * c.mu[2] - 4.0 * c.mu[3]) + e.r1 * (4.0 * sj[3] - 2.0 * sj[2]));
    }
    pos0_bar[prob] = ok ? -dx0_bar : nan;
    pos1_bar[prob] = ok ? dx0_bar - dx1_bar : nan;
    pos2_bar[prob] = ok ? dx1_bar : nan;
    if constexpr (Vel) {
        vel0_bar[prob] = ok ? v0_bar : nan;
        vel2_bar[prob] = ok ? v2_bar : nan;
    }
}

// x_dot = J theta_dot.  Vel: with the tangents of vel0 and vel2 (otherwise not read).
template <bool Vel>
__device__ __forceinline__ void solution_jvp(const double *base, size_t stride, size_t n, const uint32_t *prob_of, double limit,
                                             const double *t_pos0, const double *t_pos1, const double *t_pos2, const double *t_vel0,
                                             const double *t_vel2, double *t_vel1, double *t_dur0, double *t_dur1)
{
    double f[16];
    size_t prob;
    if (!load_lane(base, stride, n, prob_of, f, prob)) return;
    const double tp0 = t_pos0 ? t_pos0[prob] : 0.0, tp1 = t_pos1 ? t_pos1[prob] : 0.0, tp2 = t_pos2 ? t_pos2[prob] : 0.0;
    const double tv0 = Vel && t_vel0 ? t_vel0[prob] : 0.0, tv2 = Vel && t_vel2 ? t_vel2[prob] : 0.0;

    Condensed c;
    const bool ok = condense_with_K<Vel>(f, limit, c);
    ddv rhs[1][3], xd[1][3];
    // equal position tangents: dX tangents of exactly 0; zero velocity tangents: the right-hand side without Vel
    forward_rhs<Vel>(c, tp1 - tp0, tp2 - tp1, tv0, tv2, rhs[0]);
    solve3_dd<1>(c.K, rhs, xd);
    const double nan = __builtin_nan("");
    t_vel1[prob] = ok ? xd[0][0].hi : nan;
    t_dur0[prob] = ok ? xd[0][1].hi : nan;
    t_dur1[prob] = ok ? xd[0][2].hi : nan;
}

// Stores what direction k's solution x = dx / d(direction k) determines of a Jacobian whose rows are `ld` apart, NaN where the state
// gets no formula.  Directions 0 and 1 are dX0 and dX1: columns pos0, pos1, pos2 through dX0 = pos1 - pos0, dX1 = pos2 - pos1, so x is
// kept in d0 at k = 0 and column pos1 is stored at k = 1.  Directions 2 and 3 (vel0, vel2) are columns 3 and 4 as they are.
template <int ld>
__device__ __forceinline__ void store_direction(double *out, int k, const double (&x)[3], double (&d0)[3], bool ok)
{
    const double nan = __builtin_nan("");
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        if (k == 0) { d0[a] = x[a]; out[ld * a + 0] = ok ? -x[a] : nan; }
        else if (k == 1) { out[ld * a + 1] = ok ? d0[a] - x[a] : nan; out[ld * a + 2] = ok ? x[a] : nan; }
        else out[ld * a + k + 1] = ok ? x[a] : nan;
    }
}

// J[a][b] = d x_a / d theta_b, row-major: 3 x 3 in the positions at jac[9 i + 3 a + b], or (Vel) 3 x 5 with b over (pos0, pos1, pos2,
// vel0, vel2) at jac[15 i + 5 a + b].  The right-hand sides of the directions dX0, dX1 (and vel0, vel2) are formed first, so that
// D_j h_j and mu_j are dead before the elimination.  The two eliminate K differently on purpose: two right-hand sides go through one
// solve3_dd (96 VGPRs); for four, K is eliminated once (lu3_dd) and applied to them one at a time, the columns stored as soon as
// they are known: 128 VGPRs (one solve3_dd on all four, or two pairs on copies of K: 134-140).
template <bool Vel>
__device__ __forceinline__ void solution_jacobian(const double *base, size_t stride, size_t n, const uint32_t *prob_of, double limit,
                                                  double *jac)
{
    double f[16];
    size_t prob;
    if (!load_lane(base, stride, n, prob_of, f, prob)) return;

    Condensed c;
    const bool ok = condense_with_K<Vel>(f, limit, c);
    constexpr int R = Vel ? 4 : 2, ld = Vel ? 5 : 3;
    ddv rhs[R][3];      // rhs[0], rhs[1]: the directions dX0, dX1
    forward_rhs<false>(c, 1.0, 0.0, 0.0, 0.0, rhs[0]);
    forward_rhs<false>(c, 0.0, 1.0, 0.0, 0.0, rhs[1]);
    double *out = jac + prob * (3 * ld);
    double d0[3];      // dx / d dX0, until dx / d dX1 is known
    if constexpr (Vel) {
        forward_rhs<true>(c, 0.0, 0.0, 1.0, 0.0, rhs[2]);
        forward_rhs<true>(c, 0.0, 0.0, 0.0, 1.0, rhs[3]);
        rhs[2][2] = rhs[3][1] = dd_of(0.0);      // a velocity enters only its own segment's duration row (the kernel cannot know these are 0)
        bool sw[3];
        lu3_dd(c.K, sw);
#pragma unroll
        for (int k = 0; k < 4; ++k) {      // one right-hand side after the other; every column stored as soon as it is known
            ddv X[3];
            lu3_dd_solve(c.K, sw, rhs[k], X);
            const double x[3] = {X[0].hi, X[1].hi, X[2].hi};
            store_direction<ld>(out, k, x, d0, ok);
        }
    } else {
        ddv d[2][3];      // d[0] = dx / d dX0, d[1] = dx / d dX1
        solve3_dd<2>(c.K, rhs, d);
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const double x[3] = {d[k][0].hi, d[k][1].hi, d[k][2].hi};
            store_direction<ld>(out, k, x, d0, ok);
        }
    }
}

// X = A^-1 B for an N x N system and R right-hand sides in float64: solve3_dd's elimination (the second-order kernel's 7 x 7).
template <int N, int R>
__device__ __forceinline__ void solve_pivoted(double (&A)[N][N], double (&B)[R][N], double (&X)[R][N])
{
#pragma unroll
    for (int k = 0; k < N - 1; ++k) {
#pragma unroll
        for (int r = k + 1; r < N; ++r) {
            const bool sw = __builtin_fabs(A[r][k]) > __builtin_fabs(A[k][k]);
#pragma unroll
            for (int c = k; c < N; ++c) {
                const double a = A[k][c], o = A[r][c];
                A[k][c] = sw ? o : a;
                A[r][c] = sw ? a : o;
            }
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const double a = B[q][k], o = B[q][r];
                B[q][k] = sw ? o : a;
                B[q][r] = sw ? a : o;
            }
        }
#pragma unroll
        for (int r = k + 1; r < N; ++r) {
            const double f = A[r][k] / A[k][k];
#pragma unroll
            for (int c = k + 1; c < N; ++c) A[r][c] -= f * A[k][c];
#pragma unroll
            for (int q = 0; q < R; ++q) B[q][r] -= f * B[q][k];
        }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
#pragma unroll
        for (int k = N - 1; k >= 0; --k) {
            double acc = B[q][k];
#pragma unroll
            for (int c = k + 1; c < N; ++c) acc -= A[k][c] * X[q][c];
            X[q][k] = acc / A[k][k];
        }
    }
}

// Second derivatives (rp_batch_solution_hessian).  For position-delta tangents u, w (the unit dX0 and dX1
// directions): M z_uw = -R_uw, R_uw the second total derivative of r along (z_u, u), (z_w, w) without the z_uw terms.  With the
// multipliers eliminated as in the VJP, on the same (double-double) K:
//     K x_uw = -T_uw - S_j h_j (D_j Q_j,uw + 2 (E_j / D_j^2) mu_j,u mu_j,w)
//     T_uw = S_j [mu_j,u h_j,w + mu_j,w h_j,u + mu_j a3_j(u, w)],    E_j = lam_p / c_p^2 - lam_m / c_m^2
// where a_j is differentiated in (v, t, dX) of its segment: Q_j,uw = y_u^T (grad^2 a_j) y_w with y_u = (v_u, t_u, dX_u), h_j,w the
// derivative of h_j along y_w, a3_j(u, w) = grad_x (grad^2 a_j)[y_u, y_w] (the non-zero third derivatives: a_ttt, a_vtt, a_Xtt).
// The pair's first-order dual step mu_j,u = D_j A_j,u is O(1), but A_j,u (the total derivative of a_j) cancels to O(p) on an
// active pair: formed from a float64 condensed x_u, eps-level errors come back multiplied by D_j.  So the first-order steps are the
// unknowns of the 7 x 7 symmetric system [[W, H^T], [H, -diag(1 / D)]] [x_u; mu_u] = [-b_x; -alpha_u] (row j: h_j . x_u -
// mu_j,u / D_j = -alpha_j,u, well scaled whether the pair is active or not), and E_j / D_j^2 -> 1 / lam on an active pair: no large
// factor is formed outside K.  The second-order right-hand sides (D_j Q_j,uw exact) go to the double-double K of the VJP.  a_j = 6 sg_j dX r^2 + w_j r (r = 1 / t, w_j the velocity combination, dw_j / dv = cv_j).
__global__ void __launch_bounds__(kVjpBlock)
k_solution_hessian(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
                   double *__restrict__ jac, double *__restrict__ hess)
{
    double f[16];
    size_t prob;
    if (!load_lane(base, stride, n, prob_of, f, prob)) return;

    Condensed c;
    const bool ok = condense(f, limit, c);
    const Acc<double> &e = c.e;
    const double v = f[0], v0 = f[12], v2 = f[15];
    const double dx[2] = {f[13] - f[11], f[14] - f[13]};
    const double wj[4] = {-4.0 * v0 - 2.0 * v, 2.0 * v0 + 4.0 * v, -4.0 * v - 2.0 * v2, 2.0 * v + 4.0 * v2};
    constexpr double sg[4] = {1.0, -1.0, 1.0, -1.0}, cv[4] = {-2.0, 4.0, -4.0, 2.0};
    double ed2[4];
    const double c_floor = limit * 8.673617379884035e-19;
#pragma unroll
    for (int j = 0; j < 4; ++j) {      // E_j / D_j^2 with the constraint values floored as D_j's are
        const double cm = max_(-c_value<double, 3>(2 * j, e, limit), c_floor), cp = max_(-c_value<double, 3>(2 * j + 1, e, limit), c_floor);
        const double d2 = c.D[j] * c.D[j];
        // A pair whose multipliers are 0, or so small that D_j^2 is 0 or below the normal range, has E_j / D_j^2 ~ 1 / lam while
        // mu_j,u mu_j,w ~ lam^2: the term is ~lam, 0 to working precision, where the quotient would be 0 / 0 or x / 0.
        ed2[j] = d2 >= 2.2250738585072014e-308 ? (f[4 + 2 * j] / (cp * cp) - f[3 + 2 * j] / (cm * cm)) / d2 : 0.0;
    }

    // first order: [[W, H^T], [H, -diag(1 / D)]] [x_u; mu_u] = [-b_x; -alpha_u] for u = dX0, dX1
    double A[7][7];
#pragma unroll
    for (int i = 0; i < 7; ++i)
#pragma unroll
        for (int k = 0; k < 7; ++k) A[i][k] = 0.0;
    A[0][1] = A[1][0] = c.W01;      // W: K's second-derivative part
    A[0][2] = A[2][0] = c.W02;
    A[1][1] = c.W11;
    A[2][2] = c.W22;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int seg = 1 + (j >> 1);
        A[0][3 + j] = A[3 + j][0] = c.gv[j];
        A[seg][3 + j] = A[3 + j][seg] = e.gt[j];
        A[3 + j][3 + j] = -1.0 / max_(c.D[j], 2.2250738585072014e-308);
    }
    double B[2][7], Z[2][7];
#pragma unroll
    for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int i = 0; i < 7; ++i) B[u][i] = 0.0;
    const double q0 = e.r0 * e.r0, q1 = e.r1 * e.r1;
    B[0][1] = -(12.0 * q0 * e.r0 * (c.mu[1] - c.mu[0]));
    B[1][2] = -(12.0 * q1 * e.r1 * (c.mu[3] - c.mu[2]));
#pragma unroll
    for (int j = 0; j < 4; ++j) B[j >> 1][3 + j] = -(6.0 * sg[j] * (j < 2 ? q0 : q1));
    solve_pivoted<7, 2>(A, B, Z);      // Z[u] = (x_u, mu_u)
    condense_K(c);

    // second order: three right-hand sides (u, w) = (0, 0), (0, 1), (1, 1) on K, from a_j's derivatives in (v, t, dX)
    double att[4], avt[4], axt[4], attt[4], avtt[4], axtt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double r = j < 2 ? e.r0 : e.r1;
        const double r2 = r * r, r3 = r2 * r, r4 = r2 * r2, u = dx[j >> 1] * r;
        att[j] = (36.0 * sg[j] * u + 2.0 * wj[j]) * r3;
        avt[j] = -cv[j] * r2;
        axt[j] = -12.0 * sg[j] * r3;
        attt[j] = -(144.0 * sg[j] * u + 6.0 * wj[j]) * r4;
        avtt[j] = 2.0 * cv[j] * r3;
        axtt[j] = 36.0 * sg[j] * r4;
    }
    double xw[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {      // one right-hand side at a time, each on a copy of K: the same pivots and arithmetic as one
        const int u = k == 2 ? 1 : 0, w = k == 0 ? 0 : 1;      // elimination on all three, in fewer registers
        ddv S[1][3] = {{dd_of(0.0), dd_of(0.0), dd_of(0.0)}}, X[1][3];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int seg = j >> 1;
            const double vu = Z[u][0], tu = Z[u][1 + seg], Xu = seg == u ? 1.0 : 0.0;
            const double vw = Z[w][0], tw = Z[w][1 + seg], Xw = seg == w ? 1.0 : 0.0;
            const double mu_u = Z[u][3 + j], mu_w = Z[w][3 + j];
            const double tt = tu * tw, vt = vu * tw + vw * tu, Xt = Xu * tw + Xw * tu;
            const double Q = att[j] * tt + avt[j] * vt + axt[j] * Xt;
            const double a3v = c.mu[j] * (avtt[j] * tt);
            const double a3t = c.mu[j] * (attt[j] * tt + avtt[j] * vt + axtt[j] * Xt);
            const double hv_u = avt[j] * tu, hv_w = avt[j] * tw;
            const double ht_u = att[j] * tu + avt[j] * vu + axt[j] * Xu, ht_w = att[j] * tw + avt[j] * vw + axt[j] * Xw;
            const ddv sj = dd_add(two_prod(c.D[j], Q), dd_of(2.0 * ed2[j] * mu_u * mu_w));      // D_j Q_j exactly: the large term
            S[0][0] = dd_sub(S[0][0], dd_add(dd_of(mu_u * hv_w + mu_w * hv_u + a3v), dd_mul_d(sj, c.gv[j])));
            S[0][1 + seg] = dd_sub(S[0][1 + seg], dd_add(dd_of(mu_u * ht_w + mu_w * ht_u + a3t), dd_mul_d(sj, e.gt[j])));
        }
        ddv K[3][3];
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) K[a][b] = c.K[a][b];
        solve3_dd<1>(K, S, X);
#pragma unroll
        for (int a = 0; a < 3; ++a) xw[k][a] = X[0][a].hi;
    }

    const double nan = __builtin_nan("");
    if (jac) {
        double *out = jac + prob * 9;
#pragma unroll
        for (int a = 0; a < 3; ++a) {      // store_direction's columns, a row at a time (through it: one s_nop fewer, not the same code)
            out[3 * a + 0] = ok ? -Z[0][a] : nan;
            out[3 * a + 1] = ok ? Z[0][a] - Z[1][a] : nan;
            out[3 * a + 2] = ok ? Z[1][a] : nan;
        }
    }
    // H[a] = P^T [[x00, x01], [x01, x11]] P, P = d(dX0, dX1) / d(pos0, pos1, pos2) = [[-1, 1, 0], [0, -1, 1]]
    double *out = hess + prob * 27;
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        const double h00 = xw[0][a], h02 = -xw[1][a], h22 = xw[2][a];
        const double h01 = xw[1][a] - xw[0][a], h12 = xw[1][a] - xw[2][a];
        const double h11 = -h01 - h12;
        const double H[6] = {h00, h01, h02, h11, h12, h22};      // (b, c) = 00, 01, 02, 11, 12, 22
        out[9 * a + 0] = ok ? H[0] : nan;
        out[9 * a + 1] = out[9 * a + 3] = ok ? H[1] : nan;
        out[9 * a + 2] = out[9 * a + 6] = ok ? H[2] : nan;
        out[9 * a + 4] = ok ? H[3] : nan;
        out[9 * a + 5] = out[9 * a + 7] = ok ? H[4] : nan;
        out[9 * a + 8] = ok ? H[5] : nan;
    }
}

// The first-order kernels: each body at its Vel, under the names and parameter lists the C ABI's entries launch.
__global__ void __launch_bounds__(kVjpBlock)
k_solution_vjp(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
               const double *__restrict__ g_vel1, const double *__restrict__ g_dur0, const double *__restrict__ g_dur1,
               double *__restrict__ pos0_bar, double *__restrict__ pos1_bar, double *__restrict__ pos2_bar)
{
    solution_vjp<false>(base, stride, n, prob_of, limit, g_vel1, g_dur0, g_dur1, pos0_bar, pos1_bar, pos2_bar, nullptr, nullptr);
}

__global__ void __launch_bounds__(kVjpBlock)
k_endvel_vjp(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
             const double *__restrict__ g_vel1, const double *__restrict__ g_dur0, const double *__restrict__ g_dur1,
             double *__restrict__ pos0_bar, double *__restrict__ pos1_bar, double *__restrict__ pos2_bar,
             double *__restrict__ vel0_bar, double *__restrict__ vel2_bar)
{
    solution_vjp<true>(base, stride, n, prob_of, limit, g_vel1, g_dur0, g_dur1, pos0_bar, pos1_bar, pos2_bar, vel0_bar, vel2_bar);
}

__global__ void __launch_bounds__(kVjpBlock)
k_solution_jvp(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
               const double *__restrict__ t_pos0, const double *__restrict__ t_pos1, const double *__restrict__ t_pos2,
               double *__restrict__ t_vel1, double *__restrict__ t_dur0, double *__restrict__ t_dur1)
{
    solution_jvp<false>(base, stride, n, prob_of, limit, t_pos0, t_pos1, t_pos2, nullptr, nullptr, t_vel1, t_dur0, t_dur1);
}

__global__ void __launch_bounds__(kVjpBlock)
k_endvel_jvp(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
             const double *__restrict__ t_pos0, const double *__restrict__ t_pos1, const double *__restrict__ t_pos2,
             const double *__restrict__ t_vel0, const double *__restrict__ t_vel2,
             double *__restrict__ t_vel1, double *__restrict__ t_dur0, double *__restrict__ t_dur1)
{
    solution_jvp<true>(base, stride, n, prob_of, limit, t_pos0, t_pos1, t_pos2, t_vel0, t_vel2, t_vel1, t_dur0, t_dur1);
}

__global__ void __launch_bounds__(kVjpBlock)
k_solution_jacobian(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
                    double *__restrict__ jac)
{
    solution_jacobian<false>(base, stride, n, prob_of, limit, jac);
}

__global__ void __launch_bounds__(kVjpBlock)
k_endvel_jacobian(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of, double limit,
                  double *__restrict__ jac)
{
    solution_jacobian<true>(base, stride, n, prob_of, limit, jac);
}

// One lane per batch position, on `stream`: the leading arguments every kernel here takes, then its own
template <typename Kernel, typename... Args>
hipError_t launch_per_problem(Kernel kernel, const BatchView &b, const HostParams &hp, hipStream_t stream, Args... args)
{
    if (b.n == 0) return hipSuccess;
    const unsigned blocks = (unsigned)((b.n + kVjpBlock - 1) / kVjpBlock);
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kVjpBlock), 0, stream, (const double *)b.base, b.stride, b.n,
                       b.scheduled ? (const uint32_t *)b.prob_of : nullptr, hp.accel_limit, args...);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_solution_vjp(const BatchView &b, const HostParams &hp, const double *d_g_vel1, const double *d_g_dur0,
                               const double *d_g_dur1, double *d_pos0_bar, double *d_pos1_bar, double *d_pos2_bar, hipStream_t stream)
{
    return launch_per_problem(k_solution_vjp, b, hp, stream, d_g_vel1, d_g_dur0, d_g_dur1, d_pos0_bar, d_pos1_bar, d_pos2_bar);
}

hipError_t launch_solution_jvp(const BatchView &b, const HostParams &hp, const double *d_t_pos0, const double *d_t_pos1,
                               const double *d_t_pos2, double *d_t_vel1, double *d_t_dur0, double *d_t_dur1, hipStream_t stream)
{
    return launch_per_problem(k_solution_jvp, b, hp, stream, d_t_pos0, d_t_pos1, d_t_pos2, d_t_vel1, d_t_dur0, d_t_dur1);
}

hipError_t launch_solution_jacobian(const BatchView &b, const HostParams &hp, double *d_jac, hipStream_t stream)
{
    return launch_per_problem(k_solution_jacobian, b, hp, stream, d_jac);
}

hipError_t launch_solution_hessian(const BatchView &b, const HostParams &hp, double *d_jac, double *d_hess, hipStream_t stream)
{
    return launch_per_problem(k_solution_hessian, b, hp, stream, d_jac, d_hess);
}

hipError_t launch_solution_vjp_vel(const BatchView &b, const HostParams &hp, const double *d_g_vel1, const double *d_g_dur0,
                                   const double *d_g_dur1, double *d_pos0_bar, double *d_pos1_bar, double *d_pos2_bar,
                                   double *d_vel0_bar, double *d_vel2_bar, hipStream_t stream)
{
    return launch_per_problem(k_endvel_vjp, b, hp, stream, d_g_vel1, d_g_dur0, d_g_dur1, d_pos0_bar, d_pos1_bar, d_pos2_bar, d_vel0_bar,
                              d_vel2_bar);
}

hipError_t launch_solution_jvp_vel(const BatchView &b, const HostParams &hp, const double *d_t_pos0, const double *d_t_pos1,
                                   const double *d_t_pos2, const double *d_t_vel0, const double *d_t_vel2, double *d_t_vel1,
                                   double *d_t_dur0, double *d_t_dur1, hipStream_t stream)
{
    return launch_per_problem(k_endvel_jvp, b, hp, stream, d_t_pos0, d_t_pos1, d_t_pos2, d_t_vel0, d_t_vel2, d_t_vel1, d_t_dur0,
                              d_t_dur1);
}

hipError_t launch_solution_jacobian_vel(const BatchView &b, const HostParams &hp, double *d_jac, hipStream_t stream)
{
    return launch_per_problem(k_endvel_jacobian, b, hp, stream, d_jac);
}

}  // namespace rp
