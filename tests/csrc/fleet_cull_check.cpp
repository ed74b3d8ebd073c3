// fleet_cull_check.cpp -- csrc/fleet_cull.h on the host, as a stand-alone program for the address and undefined-behaviour sanitizers
// (tests/test_fleet_cull_cpu.py builds and runs it).  Per number of axes d = 1, 2, 3 it feeds cull_far more than
// 10^6 pairs of boxes and checks three statements against the same bound in long double (x87: 64 bits of mantissa), formed from the same
// boxes with the slacks ignored:
//   (1) far implies that the long double bound is above the level;
//   (2) a NaN or an infinity in any box end, slack or the level gives not far;
//   (3) finite boxes with coordinates below 10^6 whose long double bound is above level (1 + 1e-6) are far -- asked where every axis with a
//       positive gap has slack_i + slack_j <= 2^-22 gap and the bound is at least 2^-1000.  Why those two conditions: the slacks take
//       (slack_i + slack_j) / gap <= 2^-22 off every gap, so at most 2^-21 (relatively) off the sum of squares, the margin 2^-40 and the
//       d + 2 roundings at most 2^-39 more, together below 4.8e-7 < 1e-6; and below 2^-1000 a square leaves the normal range, where
//       its rounding is no longer relative.  The slacks of the random boxes are the kernel's own form for a vehicle standing at the box
//       (cull_slack of three positions, no velocity), so the condition holds for every gap above 2^-11 of the coordinates.
// It prints one line per d: the cases, how many were far, how many had a non-finite input, how many met (3)'s conditions.  Exit status 0
// when every statement held; the first violation is printed and ends the run with status 1.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>

#include "fleet_cull.h"

namespace {

struct Rng {
    uint64_t s;
    uint64_t next()
    {
        s ^= s >> 12;
        s ^= s << 25;
        s ^= s >> 27;
        return s * 0x2545F4914F6CDD1Dull;
    }
    double unit() { return (double)(next() >> 11) * 0x1p-53; }                      // [0, 1)
    double between(double a, double b) { return a + (b - a) * unit(); }
    unsigned below(unsigned n) { return (unsigned)(next() % n); }
};

struct Case {
    double lo_i[3], hi_i[3], lo_j[3], hi_j[3], slack_i[3], slack_j[3], level;
};

struct Tally {
    long cases, far, nonfinite, third;
};

long double bound_ld(const Case &c, int d)
{
    long double sum = 0.0L;
    for (int x = 0; x < d; ++x) {
        const long double left = (long double)c.lo_i[x] - (long double)c.hi_j[x], right = (long double)c.lo_j[x] - (long double)c.hi_i[x];
        long double gap = left > right ? left : right;
        gap = gap > 0.0L ? gap : 0.0L;
        sum += gap * gap;
    }
    return sum;
}

bool check(const Case &c, int d, Tally &t, const char *family)
{
    rp::CullBound b = rp::cull_begin();
    for (int x = 0; x < d; ++x) rp::cull_add(b, c.lo_i[x], c.hi_i[x], c.lo_j[x], c.hi_j[x], c.slack_i[x], c.slack_j[x]);
    const bool far = rp::cull_far(b, c.level);
    bool finite = std::isfinite(c.level), small = true, thin = true;
    for (int x = 0; x < d; ++x) {
        const double v[6] = {c.lo_i[x], c.hi_i[x], c.lo_j[x], c.hi_j[x], c.slack_i[x], c.slack_j[x]};
        for (double y : v) finite = finite && std::isfinite(y);
        for (int f = 0; f < 4; ++f) small = small && std::fabs(v[f]) < 1e6;
        const double left = c.lo_i[x] - c.hi_j[x], right = c.lo_j[x] - c.hi_i[x], gap = left > right ? left : right;
        if (gap > 0.0) thin = thin && (c.slack_i[x] + c.slack_j[x]) <= 0x1p-22 * gap;
    }
    ++t.cases;
    t.far += far;
    t.nonfinite += !finite;
    if (!finite) {
        if (far) { std::printf("%s d=%d: far with a non-finite input\n", family, d); return false; }
        return true;
    }
    const long double bound = bound_ld(c, d), level = (long double)c.level;
    if (far && !(bound > level)) {
        std::printf("%s d=%d: far, but the long double bound %.21Lg is not above the level %.17g\n", family, d, bound, c.level);
        return false;
    }
    const long double room = level >= 0.0L ? level * (1.0L + 1e-6L) : level;
    if (small && thin && bound >= 0x1p-1000L && bound > room) {
        ++t.third;
        if (!far) {
            std::printf("%s d=%d: not far, but the long double bound %.21Lg is above %.17g (1 + 1e-6)\n", family, d, bound, c.level);
            return false;
        }
    }
    return true;
}

// a box pair of random place and size; slacks: the kernel's form for a vehicle standing at the box
Case random_case(Rng &r, int d, double span, double width)
{
    Case c{};
    for (int x = 0; x < 3; ++x) {
        const double a = r.between(-span, span), b = r.between(-span, span);
        c.lo_i[x] = a; c.hi_i[x] = a + r.between(0.0, width);
        c.lo_j[x] = b; c.hi_j[x] = b + r.between(0.0, width);
        c.slack_i[x] = rp::cull_slack(c.lo_i[x], c.hi_i[x], c.hi_i[x], 0.0, 0.0, 0.0, 1.0, 1.0);
        c.slack_j[x] = rp::cull_slack(c.lo_j[x], c.hi_j[x], c.hi_j[x], 0.0, 0.0, 0.0, 1.0, 1.0);
    }
    (void)d;
    c.level = 0.0;
    return c;
}

bool run(int d, Tally &t)
{
    Rng r{0x9E3779B97F4A7C15ull + (uint64_t)d};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    // random boxes at three scales, the level from nothing to beyond the boxes' spread
    for (int i = 0; i < 450000; ++i) {
        const double span = i % 3 == 0 ? 10.0 : (i % 3 == 1 ? 1000.0 : 9e5);
        Case c = random_case(r, d, span, span * 0.01);
        const double reach = r.between(0.0, span);
        c.level = reach * reach;
        if (!check(c, d, t, "random")) return false;
    }
    // the level right at the bound: (1 + u 2^-e) times the long double bound rounded to double, e from 10 to 60
    for (int i = 0; i < 150000; ++i) {
        Case c = random_case(r, d, 100.0, 1.0);
        const double at = (double)bound_ld(c, d);
        c.level = at * (1.0 + r.between(-1.0, 1.0) * std::ldexp(1.0, -(int)(10 + r.below(51))));
        if (!check(c, d, t, "at the bound")) return false;
    }
    // touching, overlapping and nested boxes; degenerate ones (min == max), also coinciding
    for (int i = 0; i < 150000; ++i) {
        Case c = random_case(r, d, 50.0, 5.0);
        for (int x = 0; x < d; ++x) {
            switch (r.below(5)) {
            case 0: c.lo_j[x] = c.hi_i[x]; c.hi_j[x] = c.lo_j[x] + r.between(0.0, 5.0); break;      // touching
            case 1: c.lo_j[x] = r.between(c.lo_i[x], c.hi_i[x]); c.hi_j[x] = c.lo_j[x] + 5.0; break;      // overlapping
            case 2: c.lo_j[x] = c.lo_i[x]; c.hi_j[x] = c.hi_i[x]; break;      // the same box
            case 3: c.hi_i[x] = c.lo_i[x]; c.hi_j[x] = c.lo_j[x]; break;      // two points
            default: c.hi_i[x] = c.lo_i[x]; c.lo_j[x] = c.hi_j[x] = c.lo_i[x]; break;      // one point
            }
        }
        const double level[6] = {0.0, -0.0, 1.0, -1.0, 0x1p-1074, r.between(0.0, 100.0)};
        c.level = level[r.below(6)];
        if (!check(c, d, t, "touching")) return false;
    }
    // gaps within 1 +- 2^-20 ... 2^-52 of the radius, in dyadic numbers: points and unit boxes a gap r (1 + s 2^-j) apart in one axis, the
    // other axes overlapping; and the same at a distance shared between the axes
    for (int i = 0; i < 150000; ++i) {
        Case c{};
        const int j = 20 + (int)r.below(33), along = (int)r.below((unsigned)d);
        const double radius = std::ldexp(1.0 + (double)r.below(1024) * 0x1p-10, (int)r.below(8) - 2);
        const double gap = radius * (1.0 + (r.below(2) ? 1.0 : -1.0) * std::ldexp(1.0, -j) * (double)r.below(2));
        const double width = r.below(2) ? 1.0 : 0.0;
        for (int x = 0; x < 3; ++x) {
            c.lo_i[x] = 0.0; c.hi_i[x] = width;
            c.lo_j[x] = x == along ? width + gap : 0.0; c.hi_j[x] = c.lo_j[x] + width;
            const bool with_slack = r.below(2);
            c.slack_i[x] = with_slack ? rp::cull_slack(c.lo_i[x], c.hi_i[x], c.hi_i[x], 0.0, 0.0, 0.0, 1.0, 1.0) : 0.0;
            c.slack_j[x] = with_slack ? rp::cull_slack(c.lo_j[x], c.hi_j[x], c.hi_j[x], 0.0, 0.0, 0.0, 1.0, 1.0) : 0.0;
        }
        if (i % 2 && d > 1) {      // a 3-4-5 split over two axes: gaps 3/4 and 1 of `gap`, the level (5/4 radius)^2
            const int other = (along + 1) % d;
            c.lo_j[along] = width + 0.75 * gap; c.hi_j[along] = c.lo_j[along] + width;
            c.lo_j[other] = width + gap; c.hi_j[other] = c.lo_j[other] + width;
            c.level = (1.25 * radius) * (1.25 * radius);
        } else {
            c.level = radius * radius;
        }
        if (!check(c, d, t, "at the radius")) return false;
    }
    // a NaN, +inf or -inf in every field in turn, on boxes that are far without it; zero, negative and infinite levels
    const double special[3] = {nan, inf, -inf};
    for (int i = 0; i < 100000; ++i) {
        Case c = random_case(r, d, 1000.0, 1.0);
        c.level = 0x1p-20;
        const int fields = 6 * d + 1, field = i % fields;
        const double value = special[(i / fields) % 3];
        double *const at[6] = {c.lo_i, c.hi_i, c.lo_j, c.hi_j, c.slack_i, c.slack_j};
        if (field == 6 * d) c.level = value; else at[field % 6][field / 6] = value;
        if (!check(c, d, t, "non-finite")) return false;
    }
    for (int i = 0; i < 50000; ++i) {
        Case c = random_case(r, d, 1000.0, 1.0);
        const double level[8] = {0.0, -0.0, -1.0, -1e300, -0x1p-1074, inf, -inf, nan};
        c.level = level[i % 8];
        if (!check(c, d, t, "levels")) return false;
    }
    // numbers at the ends of the range: gaps whose squares underflow or overflow
    for (int i = 0; i < 50000; ++i) {
        Case c{};
        const double scale = std::ldexp(1.0, i % 2 ? -(int)(400 + r.below(670)) : (int)(400 + r.below(620)));
        for (int x = 0; x < 3; ++x) {
            c.lo_i[x] = 0.0; c.hi_i[x] = scale * r.unit();
            c.lo_j[x] = c.hi_i[x] + scale * r.unit(); c.hi_j[x] = c.lo_j[x] + scale * r.unit();
        }
        c.level = r.below(3) == 0 ? 0.0 : (double)bound_ld(c, d) * r.between(0.5, 1.5);
        if (!check(c, d, t, "the ends of the range")) return false;
    }
    return true;
}

}  // namespace

int main()
{
    for (int d = 1; d <= 3; ++d) {
        Tally t{0, 0, 0, 0};
        if (!run(d, t)) return 1;
        std::printf("d=%d cases=%ld far=%ld nonfinite=%ld third=%ld\n", d, t.cases, t.far, t.nonfinite, t.third);
    }
    return 0;
}
