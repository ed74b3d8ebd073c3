// spline_core.h -- one problem's two-segment spline as the kernels that evaluate it see it (internal; trajectory.hip): the eight
// numbers, where they come from, the constants of a segment's cubic
//     acc0 = 6 (x1 - x0) / h^2 - (4 va + 2 vb) / h        jrk0 = 2 (vb - va) / h^2 - 2 acc0 / h
// with the divisions as multiplications by one refined reciprocal per segment (rcp_: IEEE 1/x), and the cubic itself
//     pos = x0 + (va + (acc0 + jrk0 s / 3) s / 2) s       vel = va + (acc0 + jrk0 s / 2) s       acc = acc0 + jrk0 s
// Every kernel that draws or evaluates a spline stages and evaluates through these: same statements, same bits (the build has
// -ffp-contract=off: the operand order written here is the arithmetic).
#pragma once

#include "ip_core.h"
#include "ip_kernels.h"

namespace rp {

namespace {

// N pointers that travel together as one kernel argument (null: not given)
template <class T, int N> struct Table { T *p[N]; };

template <int N, class T> Table<T, N> table_of(T *const *t)
{
    Table<T, N> x;
    for (int f = 0; f < N; ++f) x.p[f] = t[f];
    return x;
}

using Spline8 = Table<const double, 8>;      // pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1

__device__ __forceinline__ double quiet_nan() { return __builtin_nan(""); }

// the NaN rule: a duration that is not finite or not > 0 poisons both (then every constant of the problem, then every output)
__device__ __forceinline__ void check_durations(double &t0, double &t1)
{
    if (!(finite_(t0) && t0 > 0.0 && finite_(t1) && t1 > 0.0)) t0 = t1 = quiet_nan();
}

// one problem's eight numbers in the order the segments use them
struct Knots {
    double p0, p1, p2, v0, v2, v1, t0, t1;
    __device__ __forceinline__ void check() { check_durations(t0, t1); }
};

// where a problem's eight numbers come from: eight arrays in problem order (the stateless entries) ...
struct FromArrays {
    Spline8 s;
    __device__ __forceinline__ Knots load(size_t i) const
    {
        Knots k;
        k.p0 = s.p[0][i]; k.p1 = s.p[1][i]; k.p2 = s.p[2][i];
        k.v0 = s.p[3] ? s.p[3][i] : 0.0; k.v2 = s.p[4] ? s.p[4][i] : 0.0;
        k.v1 = s.p[5][i]; k.t0 = s.p[6][i]; k.t1 = s.p[7][i];
        return k;
    }
};

// ... a batch's fields, gathered through the slot map in the batch's storage type (ZV: the two end-velocity fields are not read) ...
template <typename S, int VARIANT, bool ZV> struct FromBatch {
    const S *base;
    size_t stride;
    const uint32_t *slot_of;
    __device__ __forceinline__ Knots load(size_t i) const
    {
        constexpr int CB = 3 + CMap<VARIANT>::NC;
        const S *f = base + (slot_of ? (size_t)slot_of[i] : i);
        Knots k;
        k.v1 = (double)f[0]; k.t0 = (double)f[1 * stride]; k.t1 = (double)f[2 * stride];
        k.p0 = (double)f[(CB + 0) * stride]; k.p1 = (double)f[(CB + 2) * stride]; k.p2 = (double)f[(CB + 3) * stride];
        k.v0 = ZV ? 0.0 : (double)f[(CB + 1) * stride]; k.v2 = ZV ? 0.0 : (double)f[(CB + 4) * stride];
        return k;
    }
};

// ... or two problem-order records: the positions the batch was given, rounded through its storage type S (what its constant fields
// hold), and the problem's solution record; zero end velocities.  Two 16-byte loads per record
template <typename S> struct FromRecords {
    const StartRecord *records;
    const Solution *sol;
    __device__ __forceinline__ Knots load(size_t i) const
    {
        typedef double v2 __attribute__((ext_vector_type(2)));
        const v2 *rec = reinterpret_cast<const v2 *>(records + i), *so = reinterpret_cast<const v2 *>(sol + i);
        const v2 ra = rec[0], rb = rec[1], sa = so[0], sb = so[1];
        Knots k;
        k.p0 = (double)(S)ra[0]; k.p1 = (double)(S)ra[1]; k.p2 = (double)(S)rb[0];
        k.v1 = sa[0]; k.t0 = sa[1]; k.t1 = sb[0];
        k.v0 = 0.0; k.v2 = 0.0;
        return k;
    }
};

// the constants of one segment: ih = 1 / h (rcp_)
__device__ __forceinline__ void segment_constants(double x0, double x1, double va, double vb, double ih, double &acc0, double &jrk0)
{
    const double ih2 = ih * ih;
    acc0 = (x1 - x0) * (6.0 * ih2) - (va * 4.0 + vb * 2.0) * ih;
    jrk0 = (vb - va) * (2.0 * ih2) - acc0 * (2.0 * ih);
}

// the cubic of one segment at local time s, in the constants above
__device__ __forceinline__ double cubic_pos(double x0, double va, double acc0, double jrk0, double s)
{
    return x0 + (va + (acc0 + jrk0 * (s * (1.0 / 3.0))) * (s * 0.5)) * s;
}

__device__ __forceinline__ double cubic_vel(double va, double acc0, double jrk0, double s) { return va + (acc0 + jrk0 * (s * 0.5)) * s; }

__device__ __forceinline__ double cubic_acc(double acc0, double jrk0, double s) { return acc0 + jrk0 * s; }

}  // namespace

}  // namespace rp
