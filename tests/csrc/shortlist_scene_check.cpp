// shortlist_scene_check.cpp -- the scenes of tests/shortlist_patterns.py through csrc/fleet_cull.h on the host (tests/test_shortlist_cpu.py
// builds and runs it).  The shortlist's tests choose, pair by pair, what the sieve keeps: by the level alone, on
// vehicles whose boxes are known.  This program confirms the three statements that choice rests on, with the slacks cull_slack gives:
//   standing vehicles 10 and 20 apart (boxes that are points) are far at the level 1, not far at 400 and not far at NaN;
//   a vehicle that runs from 10 towards one standing at 0 at v = 1 .. 2 over the window [0, 0.5] (box [10 - v / 2, 10]) is far at the
//   level 1 and not far at 9.6^2 .. 9.9^2.
// One line per statement; exit status 0 when all held.
#include <cmath>
#include <cstdio>
#include <limits>

#include "fleet_cull.h"

namespace {

bool far(double lo_i, double hi_i, double slack_i, double lo_j, double hi_j, double slack_j, double level)
{
    rp::CullBound b = rp::cull_begin();
    rp::cull_add(b, lo_i, hi_i, lo_j, hi_j, slack_i, slack_j);
    return rp::cull_far(b, level);
}

int failures = 0;

void expect(bool got, bool want, const char *what, double a, double level)
{
    std::printf("%s %g, level %g: %s\n", what, a, level, got ? "far" : "not far");
    if (got != want) {
        std::printf("  expected %s\n", want ? "far" : "not far");
        ++failures;
    }
}

}  // namespace

int main()
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    const double at[3] = {0.0, 10.0, 20.0};
    double slack[3];
    for (int v = 0; v < 3; ++v) slack[v] = rp::cull_slack(at[v], at[v], at[v], 0.0, 0.0, 0.0, 1.0, 1.0);
    if (!(slack[2] <= 0x1p-36 * 60.0)) { std::printf("the slack of a vehicle standing at 20 is %g\n", slack[2]); ++failures; }
    for (int i = 0; i < 3; ++i)
        for (int j = i + 1; j < 3; ++j) {
            const double apart = at[j] - at[i];
            expect(far(at[i], at[i], slack[i], at[j], at[j], slack[j], 1.0), true, "standing, apart", apart, 1.0);
            expect(far(at[i], at[i], slack[i], at[j], at[j], slack[j], 400.0), false, "standing, apart", apart, 400.0);
            expect(far(at[i], at[i], slack[i], at[j], at[j], slack[j], nan), false, "standing, apart", apart, nan);
            expect(far(at[j], at[j], slack[j], at[i], at[i], slack[i], 1.0), true, "standing, the other way round, apart", apart, 1.0);
        }
    const double speeds[5] = {1.0, 1.25, 1.5, std::nextafter(2.0, 0.0), 2.0};
    for (double v : speeds) {
        const double s = rp::cull_slack(10.0, 10.0 - v, 10.0 - 2.0 * v, -v, -v, -v, 1.0, 1.0);
        expect(far(0.0, 0.0, slack[0], 10.0 - 0.5 * v, 10.0, s, 1.0), true, "approaching at", v, 1.0);
        expect(far(0.0, 0.0, slack[0], 10.0 - 0.5 * v, 10.0, s, 9.6 * 9.6), false, "approaching at", v, 9.6 * 9.6);
        expect(far(0.0, 0.0, slack[0], 10.0 - 0.5 * v, 10.0, s, 9.9 * 9.9), false, "approaching at", v, 9.9 * 9.9);
    }
    std::printf("failures=%d\n", failures);
    return failures ? 1 : 0;
}
