// fleet_cull.h -- the broad phase of the fleet contact query (internal; trajectory.hip, and the host: it includes nothing and compiles as
// plain C++).  A vehicle's position over a window lies in a box, one [min, max] per axis; two vehicles whose boxes
// are further apart than the level cannot be within it.  This file is that bound's arithmetic and nothing else: a lower bound of the
// squared distance of two boxes, made smaller by each vehicle's slack and by a relative margin, and the decision `far`.
#pragma once

#if defined(__HIPCC__)
#define RP_CULL_INLINE __host__ __device__ __forceinline__
#else
#define RP_CULL_INLINE inline
#endif

namespace rp {

constexpr double kCullSlackUnit = 0x1p-36;      // a vehicle's slack: this times the size of its spline's numbers (cull_slack)
constexpr double kCullDeflate = 1.0 - 0x1p-40;  // the margin on the sum of squares: a thousand times the d + 2 roundings of the sum itself

RP_CULL_INLINE bool cull_finite(double x) { return x - x == 0.0; }      // false for NaN, +inf and -inf
RP_CULL_INLINE double cull_abs(double x) { return x < 0.0 ? -x : x; }

// The slack of one spline: 2^-36 (|pos0| + |pos1| + |pos2| + (|vel0| + |vel1| + |vel2|) (duration0 + duration1)) -- 2^10 times the
// 2^-46 of that size by which, at the most, the evaluator's position can leave the computed box (section 30: 2^-47 for the evaluator's
// rounding and 2^-47 for the box ends').  NaN or infinite numbers give a NaN or infinite slack.
RP_CULL_INLINE double cull_slack(double pos0, double pos1, double pos2, double vel0, double vel1, double vel2, double duration0,
                                 double duration1)
{
    const double reach = (cull_abs(vel0) + cull_abs(vel1) + cull_abs(vel2)) * (duration0 + duration1);
    return kCullSlackUnit * (cull_abs(pos0) + cull_abs(pos1) + cull_abs(pos2) + reach);
}

// One axis' share of the bound: the gap between [min_i, max_i] and [min_j, max_j], less both slacks, not below zero, squared.
// All six numbers finite (the caller's business: cull_far checks).
RP_CULL_INLINE double cull_axis(double min_i, double max_i, double min_j, double max_j, double slack_i, double slack_j)
{
    const double left = min_i - max_j, right = min_j - max_i;      // at most one is positive for min <= max
    double gap = left > right ? left : right;
    gap = gap > 0.0 ? gap : 0.0;
    gap = gap - (slack_i + slack_j);
    gap = gap > 0.0 ? gap : 0.0;
    return gap * gap;
}

// The running decision over the axes of one query, in axis order.
struct CullBound {
    double sum;
    bool finite;
};

RP_CULL_INLINE CullBound cull_begin() { return CullBound{0.0, true}; }

RP_CULL_INLINE void cull_add(CullBound &b, double min_i, double max_i, double min_j, double max_j, double slack_i, double slack_j)
{
    b.finite = b.finite && cull_finite(min_i) && cull_finite(max_i) && cull_finite(min_j) && cull_finite(max_j) && cull_finite(slack_i) &&
               cull_finite(slack_j);
    b.sum = b.sum + cull_axis(min_i, max_i, min_j, max_j, slack_i, slack_j);
}

// The lower bound that is compared with the level: the sum, deflated.
RP_CULL_INLINE double cull_bound(const CullBound &b) { return b.sum * kCullDeflate; }

// far: the two vehicles cannot be within `level` (squared distance) of each other anywhere in the window.  Any NaN or infinity among the
// box ends, the slacks, the level or the sum itself: not far -- the search decides those.
RP_CULL_INLINE bool cull_far(const CullBound &b, double level)
{
    return b.finite && cull_finite(level) && cull_finite(b.sum) && cull_bound(b) > level;
}

}  // namespace rp
