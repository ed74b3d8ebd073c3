// sensitivity_core.h -- the building blocks of the F3 derivative kernels (sensitivity.hip): double-double arithmetic, the 3 x 3
// double-double elimination (whole, and split into factor and apply), the condensed system at one state and the forward right-hand
// side of the position and end-velocity directions.  The derivation is in sensitivity.hip's opening comment and DESIGN.md section 12.
#pragma once

#include "ip_core.h"

namespace rp {

namespace {

constexpr int kVjpBlock = 256;

// Double-double arithmetic: a value is hi + lo, the pair's sum exact, ~106 significant bits -- for the condensed K, whose
// D_j h_j h_j^T part reaches ~1e12 (gap 1e-8) to ~1e17 (gap 1e-13, |c| floored) times W; in float64 the component of the solution
// in the null space of the active rows, which W alone determines, would be lost in the rounding of K (see the block comment
// further down).  two_sum, quick_two_sum and two_prod are the error-free transformations; the sums are the accurate (not the
// sloppy) double-double addition, since the elimination cancels.
struct ddv {
    double hi, lo;
};

__device__ __forceinline__ ddv two_sum(double a, double b)
{
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}

__device__ __forceinline__ ddv quick_two_sum(double a, double b)
{
    const double s = a + b;
    return {s, b - (s - a)};
}

__device__ __forceinline__ ddv two_prod(double a, double b)      // a * b exactly
{
    const double p = a * b;
    return {p, __builtin_fma(a, b, -p)};
}

__device__ __forceinline__ ddv dd_add(ddv x, ddv y)
{
    const ddv s = two_sum(x.hi, y.hi), t = two_sum(x.lo, y.lo);
    const ddv u = quick_two_sum(s.hi, s.lo + t.hi);
    return quick_two_sum(u.hi, u.lo + t.lo);
}

__device__ __forceinline__ ddv dd_neg(ddv x) { return {-x.hi, -x.lo}; }
__device__ __forceinline__ ddv dd_sub(ddv x, ddv y) { return dd_add(x, dd_neg(y)); }
__device__ __forceinline__ ddv dd_of(double a) { return {a, 0.0}; }

__device__ __forceinline__ ddv dd_mul_d(ddv x, double c)
{
    const ddv p = two_prod(x.hi, c);
    return quick_two_sum(p.hi, p.lo + x.lo * c);
}

__device__ __forceinline__ ddv dd_mul(ddv x, ddv y)
{
    const ddv p = two_prod(x.hi, y.hi);
    return quick_two_sum(p.hi, p.lo + (x.hi * y.lo + x.lo * y.hi));
}

__device__ __forceinline__ ddv dd_div(ddv x, ddv y)
{
    const double q1 = x.hi / y.hi;
    const ddv r = dd_sub(x, dd_mul_d(y, q1));
    return quick_two_sum(q1, r.hi / y.hi);
}

// X = K^-1 B for the 3 x 3 double-double K and R right-hand sides: Gaussian elimination with partial pivoting (on the high
// parts), every operation in double-double.  Each row below k is compared with row k in turn and swapped in when larger, so row k
// ends with the column's largest magnitude; the swaps are selects on registers (a dynamically indexed row would go to scratch).
template <int R>
__device__ __forceinline__ void solve3_dd(ddv (&A)[3][3], ddv (&B)[R][3], ddv (&X)[R][3])
{
#pragma unroll
    for (int k = 0; k < 2; ++k) {
#pragma unroll
        for (int r = k + 1; r < 3; ++r) {
            const bool sw = __builtin_fabs(A[r][k].hi) > __builtin_fabs(A[k][k].hi);
#pragma unroll
            for (int c = k; c < 3; ++c) {
                const ddv a = A[k][c], o = A[r][c];
                A[k][c] = sw ? o : a;
                A[r][c] = sw ? a : o;
            }
#pragma unroll
            for (int q = 0; q < R; ++q) {
                const ddv a = B[q][k], o = B[q][r];
                B[q][k] = sw ? o : a;
                B[q][r] = sw ? a : o;
            }
        }
#pragma unroll
        for (int r = k + 1; r < 3; ++r) {
            const ddv f = dd_div(A[r][k], A[k][k]);
#pragma unroll
            for (int c = k + 1; c < 3; ++c) A[r][c] = dd_sub(A[r][c], dd_mul(f, A[k][c]));
#pragma unroll
            for (int q = 0; q < R; ++q) B[q][r] = dd_sub(B[q][r], dd_mul(f, B[q][k]));
        }
    }
#pragma unroll
    for (int q = 0; q < R; ++q) {
#pragma unroll
        for (int k = 2; k >= 0; --k) {
            ddv acc = B[q][k];
#pragma unroll
            for (int c = k + 1; c < 3; ++c) acc = dd_sub(acc, dd_mul(A[k][c], X[q][c]));
            X[q][k] = dd_div(acc, A[k][k]);
        }
    }
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

// The condensed system at one state (the 16 fields of a lane): the pair weights D_j and mu_j, h_j = (gv_j, e.gt_j), the exact
// products D_j h_j and K = W + S_j D_j h_j h_j^T in double-double (condense_K); returns whether the state gets the formula or NaN.
struct Condensed {
    Acc<double> e;
    double D[4], mu[4], gv[4];
    double W01, W02, W11, W22;      // W = S_j mu_j grad^2 a_j: W(v, v) = W(t0, t1) = 0
    ddv Dgv[4], Dgt[4];             // D_j gv_j, D_j gt_j
    ddv K[3][3];
};

__device__ __forceinline__ bool condense(const double (&f)[16], double limit, Condensed &c)
{
    const double v = f[0], t0 = f[1], t1 = f[2];
    const double *lam = f + 3;
    Prob<double> k;
    k.v0 = f[12];
    k.v2 = f[15];
    k.dx0 = f[13] - f[11];
    k.dx1 = f[14] - f[13];
    Acc<double> &e = c.e;
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
    double (&D)[4] = c.D, (&mu)[4] = c.mu, (&gv)[4] = c.gv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double cm = c_value<double, 3>(2 * j, e, limit), cp = c_value<double, 3>(2 * j + 1, e, limit);
        const double lm = lam[2 * j], lp = lam[2 * j + 1];
        ok = ok && !(cm > 0.0) && !(cp > 0.0);
        D[j] = lp / max_(-cp, c_floor) + lm / max_(-cm, c_floor);
        mu[j] = lp - lm;      // S lam_i g_i = (lp - lm) grad a_j: the pair's weight in W = S lam_i H_i
        gv[j] = acc_gv(e, j);
    }
    c.W01 = mu[0] * htv[0] + mu[1] * htv[1];
    c.W02 = mu[2] * htv[2] + mu[3] * htv[3];
    c.W11 = mu[0] * htt[0] + mu[1] * htt[1];
    c.W22 = mu[2] * htt[2] + mu[3] * htt[3];
    return ok;
}

// K = W + S_j D_j h_j h_j^T in (vel1, duration0, duration1) and the products D_j h_j, in double-double
__device__ __forceinline__ void condense_K(Condensed &c)
{
    const Acc<double> &e = c.e;
    const double (&gv)[4] = c.gv;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c.Dgv[j] = two_prod(c.D[j], gv[j]);
        c.Dgt[j] = two_prod(c.D[j], e.gt[j]);
    }

    // K = W + S_j D_j h_j h_j^T in (vel1, duration0, duration1); K(t0, t1) = 0 (no constraint touches both durations)
    ddv (&K)[3][3] = c.K;
    K[0][0] = dd_mul_d(c.Dgv[0], gv[0]);
#pragma unroll
    for (int j = 1; j < 4; ++j) K[0][0] = dd_add(K[0][0], dd_mul_d(c.Dgv[j], gv[j]));
    K[0][1] = dd_add(dd_of(c.W01), dd_add(dd_mul_d(c.Dgv[0], e.gt[0]), dd_mul_d(c.Dgv[1], e.gt[1])));
    K[0][2] = dd_add(dd_of(c.W02), dd_add(dd_mul_d(c.Dgv[2], e.gt[2]), dd_mul_d(c.Dgv[3], e.gt[3])));
    K[1][1] = dd_add(dd_of(c.W11), dd_add(dd_mul_d(c.Dgt[0], e.gt[0]), dd_mul_d(c.Dgt[1], e.gt[1])));
    K[2][2] = dd_add(dd_of(c.W22), dd_add(dd_mul_d(c.Dgt[2], e.gt[2]), dd_mul_d(c.Dgt[3], e.gt[3])));
    K[1][0] = K[0][1];
    K[2][0] = K[0][2];
    K[1][2] = K[2][1] = dd_of(0.0);
}

// Both for a first-order kernel.  Vel: the derivatives with end velocities give NaN for a non-positive duration besides.
template <bool Vel>
__device__ __forceinline__ bool condense_with_K(const double (&f)[16], double limit, Condensed &c)
{
    bool ok = condense(f, limit, c);
    if constexpr (Vel) ok = ok && f[1] > 0.0 && f[2] > 0.0;
    condense_K(c);
    return ok;
}

// One lane per problem, walking batch positions: the lane's 16 fields, read coalesced, and the problem at its position, where its
// inputs are gathered and its results scattered.  False for the lanes past the end of the batch.
__device__ __forceinline__ bool load_lane(const double *__restrict__ base, size_t stride, size_t n, const uint32_t *__restrict__ prob_of,
                                          double (&f)[16], size_t &prob)
{
    const size_t s = (size_t)blockIdx.x * kVjpBlock + threadIdx.x;
    if (s >= n) return false;
#pragma unroll
    for (int i = 0; i < 16; ++i) f[i] = __builtin_nontemporal_load(base + (size_t)i * stride + s);
    prob = prob_of ? (size_t)prob_of[s] : s;
    return true;
}

// The condensed forward right-hand side -b_x - S_j D_j alpha_j h_j for position-delta tangents (dd0, dd1) = (dX0_dot, dX1_dot),
// in double-double from the exact D_j h_j: alpha_j = +-6 dd / t^2 (the tangent of a_j), and b_x = S_j mu_j beta_j with
// beta_j = -+12 dd / t^3 in the durations' rows.  Vel: of all five tangents, the end-velocity tangents (e0, e2) = (vel0_dot, vel2_dot)
// added to alpha_j and b_x before the double-double products:
//     alpha_j += (-4 e0, 2 e0) / t0, (-2 e2, 4 e2) / t1,    b_x += (0, (4 mu_0 - 2 mu_1) e0 / t0^2, (2 mu_2 - 4 mu_3) e2 / t1^2).
// With e0 = e2 = 0 the additions are of zeros, the values those without Vel bit for bit; without Vel the terms are not formed at all.
template <bool Vel>
__device__ __forceinline__ void forward_rhs(const Condensed &c, double dd0, double dd1, double e0, double e2, ddv (&rhs)[3])
{
    const Acc<double> &e = c.e;
    const double q0 = e.r0 * e.r0, q1 = e.r1 * e.r1;
    const double a0 = 6.0 * q0 * dd0, a1 = 6.0 * q1 * dd1;
    const double al[4] = {Vel ? a0 + -4.0 * e.r0 * e0 : a0, Vel ? -a0 + 2.0 * e.r0 * e0 : -a0,
                          Vel ? a1 + -2.0 * e.r1 * e2 : a1, Vel ? -a1 + 4.0 * e.r1 * e2 : -a1};
    rhs[0] = dd_neg(dd_add(dd_add(dd_mul_d(c.Dgv[0], al[0]), dd_mul_d(c.Dgv[1], al[1])),
                           dd_add(dd_mul_d(c.Dgv[2], al[2]), dd_mul_d(c.Dgv[3], al[3]))));
    const double b0 = 12.0 * q0 * e.r0 * dd0 * (c.mu[1] - c.mu[0]);
    rhs[1] = dd_neg(dd_add(dd_of(Vel ? b0 + q0 * e0 * (4.0 * c.mu[0] - 2.0 * c.mu[1]) : b0),
                           dd_add(dd_mul_d(c.Dgt[0], al[0]), dd_mul_d(c.Dgt[1], al[1]))));
    const double b1 = 12.0 * q1 * e.r1 * dd1 * (c.mu[3] - c.mu[2]);
    rhs[2] = dd_neg(dd_add(dd_of(Vel ? b1 + q1 * e2 * (2.0 * c.mu[2] - 4.0 * c.mu[3]) : b1),
                           dd_add(dd_mul_d(c.Dgt[2], al[2]), dd_mul_d(c.Dgt[3], al[3]))));
}

}  // namespace

}  // namespace rp
