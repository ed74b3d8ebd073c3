// staggered_cull_check.cpp -- the staggered half of csrc/fleet_cull.h on the host, as a stand-alone program for the address and
// undefined-behaviour sanitizers (tests/test_staggered_cull_cpu.py builds and runs it).  Per number of axes
// d = 1, 2, 3 it draws more than 10^6 tuples (two starts, a window, a level, the 2 d total times, boxes, slacks and speed bounds) and
// checks four statements:
//   (1) cull_refused, fed the way k_winnow feeds it, equals a plain restatement of contact_query's window test on the same doubles;
//   (2) a query that is far (cull_add_staggered, cull_far) has the long double bound above the level when every gap is first made
//       smaller by (speed_i + speed_j) times the time error 6 u (T_i + T_j) of section 31, u = 2^-53, and by nothing else;
//   (3) a NaN or an infinity in any box end, slack, speed bound, total time or the level gives not far;
//   (4) the time error itself: for a query that is not refused, the second vehicle's times at the two ends of the search's window,
//       fl(a - delay) and fl(b - delay), lie in [0, T_j,c + e] and, where that end of its own box window [fl(lo - s_j), fl(hi - s_j)]
//       is inside (0, T_j,c), within e of it, e = 6 u (T_i,c + T_j,c), for every axis c -- in long double.  fl(t - delay) does not
//       decrease with t, so the two ends bound every time between them.
// It prints one line per d: the cases, how many were refused, far, had a non-finite input, and went through (4).  Exit status 0 when
// every statement held; the first violation is printed and ends the run with status 1.
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
    double unit() { return (double)(next() >> 11) * 0x1p-53; }      // [0, 1)
    double between(double a, double b) { return a + (b - a) * unit(); }
    unsigned below(unsigned n) { return (unsigned)(next() % n); }
};

struct Case {
    double s_i, s_j, lo, hi, level, T_i[3], T_j[3];
    double lo_i[3], hi_i[3], lo_j[3], hi_j[3], slack_i[3], slack_j[3], speed_i[3], speed_j[3];
};

struct Tally {
    long cases, refused, far, nonfinite, timed;
};

// contact_query's window test, restated: the query has no time at which both vehicles are under way inside its window
bool refused_plain(const Case &c, int d)
{
    const double delay = c.s_j - c.s_i, lo = c.lo - c.s_i, hi = c.hi - c.s_i;
    double E = std::numeric_limits<double>::infinity();
    bool whole = true;
    for (int x = 0; x < d; ++x) {
        if (std::isnan(c.T_i[x])) whole = false;
        if (c.T_i[x] < E) E = c.T_i[x];
    }
    for (int x = 0; x < d; ++x) {
        const double end = delay + c.T_j[x];
        if (std::isnan(end)) whole = false;
        if (end < E) E = end;
    }
    const double S = delay > 0.0 ? delay : 0.0;
    double a = S, b = E;
    if (std::isnan(lo) || lo > S) a = lo;
    if (std::isnan(hi) || hi < E) b = hi;
    if (!(a <= b)) return true;
    return !(std::isfinite(delay) && std::isfinite(c.level) && whole);
}

const long double kU = 0x1p-53L;

bool check(const Case &c, int d, Tally &t, const char *family)
{
    const double delay = c.s_j - c.s_i, lo = c.lo - c.s_i, hi = c.hi - c.s_i;      // as k_winnow forms them
    rp::CullDomain w = rp::cull_domain_begin();
    for (int x = 0; x < d; ++x) rp::cull_domain_first(w, c.T_i[x]);
    for (int x = 0; x < d; ++x) rp::cull_domain_second(w, delay, c.T_j[x]);
    const bool refused = rp::cull_refused(w, delay, c.level, lo, hi);
    ++t.cases;
    t.refused += refused;
    if (refused != refused_plain(c, d)) {
        std::printf("%s d=%d: cull_refused says %d, the restatement %d (starts %.17g %.17g, window %.17g %.17g)\n", family, d, (int)refused,
                    (int)!refused, c.s_i, c.s_j, c.lo, c.hi);
        return false;
    }
    rp::CullBound b = rp::cull_begin();
    for (int x = 0; x < d; ++x)
        rp::cull_add_staggered(b, c.lo_i[x], c.hi_i[x], c.lo_j[x], c.hi_j[x], c.slack_i[x], c.slack_j[x], c.speed_i[x], c.speed_j[x], c.T_i[x],
                               c.T_j[x]);
    const bool far = rp::cull_far(b, c.level);
    t.far += far;
    bool finite = std::isfinite(c.level);
    for (int x = 0; x < d; ++x) {
        const double v[10] = {c.lo_i[x], c.hi_i[x], c.lo_j[x], c.hi_j[x], c.slack_i[x], c.slack_j[x], c.speed_i[x], c.speed_j[x], c.T_i[x], c.T_j[x]};
        for (double y : v) finite = finite && std::isfinite(y);
    }
    t.nonfinite += !finite;
    if (!finite && far) { std::printf("%s d=%d: far with a non-finite input\n", family, d); return false; }
    if (far) {
        long double sum = 0.0L;
        for (int x = 0; x < d; ++x) {
            const long double left = (long double)c.lo_i[x] - (long double)c.hi_j[x], right = (long double)c.lo_j[x] - (long double)c.hi_i[x];
            long double gap = left > right ? left : right;
            const long double theta = 6.0L * kU * ((long double)c.T_i[x] + (long double)c.T_j[x]);
            gap -= ((long double)c.speed_i[x] + (long double)c.speed_j[x]) * theta;
            gap = gap > 0.0L ? gap : 0.0L;
            sum += gap * gap;
        }
        if (!(sum > (long double)c.level)) {
            std::printf("%s d=%d: far, but the long double bound less the drift, %.21Lg, is not above the level %.17g\n", family, d, sum, c.level);
            return false;
        }
    }
    if (refused || !finite || !std::isfinite(c.s_i) || !std::isfinite(c.s_j)) return true;
    // (4): the search's window [a, b] on the first vehicle's clock, and where its ends put the second vehicle
    const double S = delay > 0.0 ? delay : 0.0;
    const double a = lo > S ? lo : S, e = hi < w.E ? hi : w.E;
    const double own_lo = c.lo - c.s_j, own_hi = c.hi - c.s_j;      // the second vehicle's box window, before its clamp
    ++t.timed;
    for (int x = 0; x < d; ++x) {
        const long double room = 6.0L * kU * ((long double)c.T_i[x] + (long double)c.T_j[x]), T = (long double)c.T_j[x];
        const double ends[2] = {a - delay, e - delay};
        for (double tau : ends) {
            bool ok = (long double)tau >= 0.0L && (long double)tau <= T + room;
            if (own_lo > 0.0 && (long double)own_lo < T) ok = ok && (long double)tau >= (long double)own_lo - room;
            if (own_hi > 0.0 && (long double)own_hi < T) ok = ok && (long double)tau <= (long double)own_hi + room;
            if (!ok) {
                std::printf("%s d=%d axis %d: the second vehicle's time %.17g leaves [0, %.17g] and [%.17g, %.17g] by more than %.3Lg\n", family, d, x,
                            tau, c.T_j[x], own_lo, own_hi, room);
                return false;
            }
        }
    }
    return true;
}

Case random_case(Rng &r, double base, double scale)
{
    Case c{};
    const double spread = r.below(2) ? 2.0 : 8.0;
    c.s_i = base + scale * r.between(0.0, spread);
    c.s_j = base + scale * r.between(0.0, spread);
    const double first = base + scale * r.between(-1.0, spread + 4.0), second = base + scale * r.between(-1.0, spread + 4.0);
    c.lo = first < second ? first : second;
    c.hi = first < second ? second : first;
    if (r.below(4) == 0) c.lo = -std::numeric_limits<double>::infinity();
    if (r.below(4) == 0) c.hi = std::numeric_limits<double>::infinity();
    for (int x = 0; x < 3; ++x) {
        c.T_i[x] = scale * r.between(0.1, 4.0);
        c.T_j[x] = scale * r.between(0.1, 4.0);
        const double p = r.between(-30.0, 30.0), q = r.between(-30.0, 30.0);
        c.lo_i[x] = p; c.hi_i[x] = p + r.between(0.0, 3.0);
        c.lo_j[x] = q; c.hi_j[x] = q + r.between(0.0, 3.0);
        c.speed_i[x] = r.between(0.0, 60.0) / scale;
        c.speed_j[x] = r.between(0.0, 60.0) / scale;
        c.slack_i[x] = rp::cull_slack(c.lo_i[x], c.hi_i[x], c.hi_i[x], c.speed_i[x], c.speed_i[x], c.speed_i[x], c.T_i[x] * 0.5, c.T_i[x] * 0.5);
        c.slack_j[x] = rp::cull_slack(c.lo_j[x], c.hi_j[x], c.hi_j[x], c.speed_j[x], c.speed_j[x], c.speed_j[x], c.T_j[x] * 0.5, c.T_j[x] * 0.5);
    }
    const double reach = r.between(0.0, 40.0);
    c.level = reach * reach;
    return c;
}

bool run(int d, Tally &t)
{
    Rng r{0xD1B54A32D192ED03ull + (uint64_t)d};
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    const double bases[6] = {0.0, 0.0, 1000.0, 0x1p20, 0x1p40, -0x1p40};
    // starts and windows at every size of start and of time
    for (int i = 0; i < 700000; ++i) {
        const Case c = random_case(r, bases[i % 6], std::ldexp(1.0, (int)r.below(21) - 10));
        if (!check(c, d, t, "random")) return false;
    }
    // the domains touch: s_j = s_i + the least T_i (rounded) and its neighbours; s_i = s_j + the least T_j and its neighbours; the window
    // ends on the starts and on the ends of the vehicles' times
    for (int i = 0; i < 200000; ++i) {
        Case c = random_case(r, bases[i % 6], std::ldexp(1.0, (int)r.below(21) - 10));
        double least_i = c.T_i[0], least_j = c.T_j[0];
        for (int x = 1; x < d; ++x) {
            least_i = c.T_i[x] < least_i ? c.T_i[x] : least_i;
            least_j = c.T_j[x] < least_j ? c.T_j[x] : least_j;
        }
        const double nudge[3] = {0.0, inf, -inf};
        if (i % 2) c.s_j = std::nextafter(c.s_i + least_i, c.s_i + least_i + nudge[r.below(3)]);
        else c.s_i = std::nextafter(c.s_j + least_j, c.s_j + least_j + nudge[r.below(3)]);
        const double marks[6] = {c.s_i, c.s_j, c.s_i + least_i, c.s_j + least_j, -inf, inf};
        if (r.below(2)) c.lo = marks[r.below(5)];
        if (r.below(2)) c.hi = marks[r.below(6) == 4 ? 5 : r.below(4)];
        if (!check(c, d, t, "touching")) return false;
    }
    // vehicles of very different total times: the allowance's own condition (kCullTimeMost) decides
    for (int i = 0; i < 50000; ++i) {
        Case c = random_case(r, 0.0, 1.0);
        const double ratio = std::ldexp(1.0, (int)r.below(40));
        for (int x = 0; x < 3; ++x) (i % 2 ? c.T_i[x] : c.T_j[x]) *= ratio;
        c.s_j = c.s_i + r.between(-1.0, 1.0) * c.T_i[0];
        c.lo = -inf;
        c.hi = inf;
        if (!check(c, d, t, "unequal")) return false;
    }
    // a NaN, +inf or -inf in every field in turn
    const double special[3] = {nan, inf, -inf};
    for (int i = 0; i < 150000; ++i) {
        Case c = random_case(r, 0.0, 1.0);
        c.level = 0x1p-20;
        const int fields = 10 * d + 5, field = i % fields;
        const double value = special[(i / fields) % 3];
        double *const per_axis[10] = {c.lo_i, c.hi_i, c.lo_j, c.hi_j, c.slack_i, c.slack_j, c.speed_i, c.speed_j, c.T_i, c.T_j};
        double *const single[5] = {&c.s_i, &c.s_j, &c.lo, &c.hi, &c.level};
        if (field >= 10 * d) *single[field - 10 * d] = value; else per_axis[field % 10][field / 10] = value;
        if (!check(c, d, t, "non-finite")) return false;
    }
    return true;
}

}  // namespace

int main()
{
    for (int d = 1; d <= 3; ++d) {
        Tally t{0, 0, 0, 0, 0};
        if (!run(d, t)) return 1;
        std::printf("d=%d cases=%ld refused=%ld far=%ld nonfinite=%ld timed=%ld\n", d, t.cases, t.refused, t.far, t.nonfinite, t.timed);
    }
    return 0;
}
