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

// ---- a start time per vehicle ----
// Pair (i, j) of a staggered fleet is searched on vehicle i's clock: delay = s_j - s_i, the window [lo - s_i, hi - s_i].  Two tests per
// query, either of which proves its outputs NaN.  Refused: contact_query's own window test on the stored totals, operation for operation
// (additions, comparisons and selections only: nothing a compiler may contract or reorder).  Far: the box bound above, with one more
// allowance, because vehicle j is evaluated at the rounded difference t - delay, which can leave j's own box window by a time error.

constexpr double kCullTimeUnit = 0x1p-40;     // the time error allowed for: this times (T_i + T_j); 2^10 times section 31's 6 u (T_i + T_j)
constexpr double kCullStretch = 0x1p-19;      // a spline's speed bound holds this share of its total time beyond its end
constexpr double kCullTimeMost = 0x1p-20;     // the allowed time error must be within this share of either total time: else not far
constexpr double kCullInflate = 1.0 + 0x1p-20;

// contact_query's common domain of one query, gathered in its order: vehicle i's D totals first, then delay + vehicle j's D totals
struct CullDomain {
    double E;
    bool whole;
};

RP_CULL_INLINE CullDomain cull_domain_begin() { return CullDomain{__builtin_inf(), true}; }

RP_CULL_INLINE void cull_domain_first(CullDomain &w, double total_i)
{
    w.whole = w.whole && total_i == total_i;
    w.E = total_i < w.E ? total_i : w.E;
}

RP_CULL_INLINE void cull_domain_second(CullDomain &w, double delay, double total_j)
{
    const double EB = delay + total_j;
    w.whole = w.whole && EB == EB;
    w.E = EB < w.E ? EB : w.E;
}

// refused: contact_query returns its NaN before the walk.  lo, hi: the window on vehicle i's clock (lo - s_i, hi - s_i as formed there).
RP_CULL_INLINE bool cull_refused(const CullDomain &w, double delay, double level, double lo, double hi)
{
    const double S = delay > 0.0 ? delay : 0.0;
    const double a = lo > S ? lo : (lo != lo ? lo : S), b = hi < w.E ? hi : (hi != hi ? hi : w.E);
    return !(a <= b && cull_finite(delay) && cull_finite(level) && w.whole);
}

// An upper bound of |velocity| of one segment's cubic va + acc0 s + jrk0 s^2 / 2 over 0 <= s <= reach, inflated beyond its own roundings
// (five, on numbers that are not negative).
RP_CULL_INLINE double cull_segment_speed(double va, double acc0, double jrk0, double reach)
{
    return (cull_abs(va) + (cull_abs(acc0) + cull_abs(jrk0) * (reach * 0.5)) * reach) * kCullInflate;
}

// The speed bound of one spline from its two segments' evaluator constants: each segment over its own length and kCullStretch of the
// total time more (the second segment is what an evaluation just beyond the end uses).
RP_CULL_INLINE double cull_speed(double va0, double acc00, double jrk00, double h0, double va1, double acc01, double jrk01, double h1, double total)
{
    const double more = kCullStretch * total;
    const double first = cull_segment_speed(va0, acc00, jrk00, h0 + more), second = cull_segment_speed(va1, acc01, jrk01, h1 + more);
    const double top = first > second ? first : second;
    return first == first ? top : first;      // a NaN in either stays one
}

// One axis' share of the staggered bound: cull_axis with both slacks made larger by the two speed bounds times the time allowance
// kCullTimeUnit (T_i + T_j).  Not finite -- never far -- also where that allowance is not within kCullTimeMost of either total.
RP_CULL_INLINE void cull_add_staggered(CullBound &b, double min_i, double max_i, double min_j, double max_j, double slack_i, double slack_j,
                                       double speed_i, double speed_j, double total_i, double total_j)
{
    const double theta = kCullTimeUnit * (total_i + total_j);
    const double drift = (speed_i + speed_j) * theta;
    b.finite = b.finite && cull_finite(speed_i) && cull_finite(speed_j) && cull_finite(theta) && cull_finite(drift) &&
               theta <= kCullTimeMost * total_i && theta <= kCullTimeMost * total_j;
    cull_add(b, min_i, max_i, min_j, max_j, slack_i + drift, slack_j);
}

}  // namespace rp
