// trajectory.hip -- what can be asked of a solved two-segment spline, gfx950.  The families, in the order of the file:
//   evaluation at the caller's own times       k_trajectory_eval, k_batch_trajectory            DESIGN.md section 13
//   ... its first derivatives                  k_trajectory_jvp, k_trajectory_vjp               section 13
//   ... the reverse rule along a direction     k_trajectory_hvp                                 section 17
//   the first time a level is reached          k_crossing, k_batch_crossing                     section 14
//   extreme pos and vel over a window          k_extrema, k_batch_extrema                       section 15
//   integrals over a window                    k_integrals, k_batch_integrals                   section 16
//   ... their first derivatives                k_jvp_integrals, k_vjp_integrals                 section 16
//   ... the reverse rule along a direction     k_window_hvp                                     section 19
//   the extreme gap between two splines        k_gap                                            section 18
//   the tracking integrals of two splines      k_tracking                                       section 20
//   ... their first derivatives                k_tracking_jvp, k_tracking_vjp                   section 20
//   ... the reverse rule along a direction     k_pair_hvp                                       section 23
//   the first time two splines meet            k_meeting                                        section 22
//   the closest approach of two vehicles       k_separation                                     section 24
//   the first time they come within a distance k_contact                                        section 25
//   the closest approach of a fleet's pairs    k_fleet                                          section 26
//   the first contact of a fleet's pairs       k_encounter                                      section 27
//   ... both with a start time per vehicle     k_stagger, k_rendezvous                          section 28
//   ... both for one fleet against another     k_versus, k_intercept                            section 34
//   plot data on the reference's fixed grid    k_sample, k_sample_records
// The entries are include/rp_batch.h's rp_trajectory_*, rp_batch_trajectory_device, rp_batch_crossing_device, rp_batch_extrema_device,
// rp_batch_integrals_device and rp_batch_sample*; the launchers are at the end of the file.
//
// Per problem the spline is (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1) -- this order wherever eight pointers travel
// together -- and the k query times tau[i, j] (row-major n x k) count from the start of segment 0.  A query with tau < duration0
// lies in segment 0, (pos0, vel0) -> (pos1, vel1) over h = duration0 at s = tau; every other one in segment 1, (pos1, vel1) ->
// (pos2, vel2) over h = duration1 at s = tau - duration0.  The cubic is the one the reference draws (drawSegment,
// onedpath_ip.cpp:1065-1088), constants and expressions in spline_core.h.  No clamping: outside [0, duration0 + duration1] the end
// segments' cubics continue.  A problem with a duration that is not finite or not > 0 gets NaN everywhere (its constants are NaN); a
// NaN tau gives NaN for that query.
//
// The shape every family but the plot data shares.  The kernels move 8-32 B per query and ~128 B per problem and do tens of flops per
// query: streaming kernels.  A block takes P consecutive problems per trip (P a function of k alone, P k ~ 4096 queries); its first
// P threads read one problem each, do the two reciprocals (rcp_) and leave what the queries need in LDS; a barrier; the block works
// through the trip's queries; a barrier.  The grid is capped and strides over the trips.  That loop is for_each_trip.
//   The pointwise kernels (everything but the two reverse rules): the block's P k queries are consecutive elements of tau (P is even,
//     so a trip starts on a 16-byte boundary): each thread takes two at a time -- one 16-byte load, one 16-byte nontemporal store per
//     wanted output -- and finds each query's problem by carrying (problem, column) along, without a division (stream_pairs).
//   The reverse rules (k_trajectory_vjp, k_trajectory_hvp, k_vjp_integrals, k_window_hvp, k_tracking_vjp, k_pair_hvp): a problem's k queries reduce to N sums (reduce_rows).  A
//     group of G lanes (a power of two <= 64, from k alone) owns one problem at a time: lane l adds queries l, l + G, l + 2 G, ...
//     (pairs 2 l, 2 l + 1, ... as 16-byte vectors when k is even -- every row then starts on a 16-byte boundary; single elements
//     when k is odd) in that order into its own sums, the lanes combine by an xor butterfly (a + b == b + a bit for bit: every lane
//     holds the same sums), and lane 0 runs the chain rule once and leaves the problem's eight gradients in LDS (route_bars), from
//     where the block's first P threads write them (write_bars).  The order of every addition is a function of k: a problem's
//     gradient is the same bits in any batch, in any block, in every run.  No atomics.
// A null output is not written, a null gradient or tangent is not read and counts as zeros -- as the VALUE zero in the same
// expression, so that null and explicit zeros give the same bits; a null window end is -inf or +inf (load_window).
#include "ip_kernels.h"

#include <type_traits>

#include "../../include/rp_batch.h"
#include "batch_dispatch.h"
#include "fleet_cull.h"
#include "fleet_index.h"
#include "ip_core.h"
#include "spline_core.h"

namespace rp {

namespace {

constexpr int kTrajBlock = 256;
constexpr int kTrajProblems = 128;       // the most problems a block stages per trip
constexpr unsigned kTrajGridCap = 2048;  // 256 CUs x 8 blocks: the blocks stride over the rest
constexpr size_t kTrajTrip = 4096;       // queries per trip a block aims at

typedef double v2 __attribute__((ext_vector_type(2)));

using SplineBar8 = Table<double, 8>;           // the eight gradients, in Spline8's order
using Out4 = Table<double, 4>;                 // pos_min, pos_max, vel_min, vel_max | pos_int, distance, vel_sq, acc_sq
using Out2 = Table<double, 2>;                 // gap_min, gap_max
using In4 = Table<const double, 4>;

__device__ __forceinline__ int problems_here(size_t n, size_t p_first, int P)
{
    return (int)(n - p_first < (size_t)P ? n - p_first : (size_t)P);
}

// The trips of a block: stage(q, i) by the first `here` threads (problem i into place q of the block's LDS), then body(p_first, here)
// by all of them, between two barriers.
template <class Stage, class Body> __device__ __forceinline__ void for_each_trip(size_t n, int P, Stage stage, Body body)
{
    const size_t trips = (n + (size_t)P - 1) / (size_t)P;
    for (size_t trip = blockIdx.x; trip < trips; trip += gridDim.x) {
        const size_t p_first = trip * (size_t)P;
        const int here = problems_here(n, p_first, P);
        if ((int)threadIdx.x < here) stage((int)threadIdx.x, p_first + threadIdx.x);
        __syncthreads();
        body(p_first, here);
        __syncthreads();
    }
}

// The streaming loop of the pointwise kernels: the block's `here` x k queries, consecutive from element p_first * k (even), two per
// thread and trip; f(element, problem within the block, second?) handles one query, g(pair) moves a pair's 16 bytes.
// (problem, column) of a thread's first query of the pair come from one division per trip and are carried from pair to pair.
template <class Pair> __device__ __forceinline__ void stream_pairs(int here, size_t k, Pair pair)
{
    const size_t count = (size_t)here * k;
    const uint32_t step = 2 * kTrajBlock, k32 = (uint32_t)k;      // k < 2^31 (the entries refuse more): 32-bit problem and column
    const uint32_t dq = step / k32, dr = step - dq * k32;          // uniform
    size_t e = 2 * (size_t)threadIdx.x;
    uint32_t q = (uint32_t)e / k32, r = (uint32_t)e - q * k32;
    for (; e + 1 < count; e += step) {
        pair(e, (int)q, (int)(r + 1 == k32 ? q + 1 : q), true);
        q += dq;
        r += dr;
        if (r >= k32) { r -= k32; ++q; }
    }
    if (e < count) pair(e, (int)q, (int)q, false);      // the last query of an odd total (the last trip of the launch only)
}

// ---- forward ----
struct EvalLds {
    double c[2][4][kTrajProblems];      // per segment: x0, va, acc0, jrk0
    double d0[kTrajProblems];
};

__device__ __forceinline__ void stage_eval(EvalLds &L, int q, Knots kn)
{
    kn.check();
    const double ih0 = rcp_<double>(kn.t0), ih1 = rcp_<double>(kn.t1);
    double acc0, jrk0;
    segment_constants(kn.p0, kn.p1, kn.v0, kn.v1, ih0, acc0, jrk0);
    L.c[0][0][q] = kn.p0; L.c[0][1][q] = kn.v0; L.c[0][2][q] = acc0; L.c[0][3][q] = jrk0;
    segment_constants(kn.p1, kn.p2, kn.v1, kn.v2, ih1, acc0, jrk0);
    L.c[1][0][q] = kn.p1; L.c[1][1][q] = kn.v1; L.c[1][2][q] = acc0; L.c[1][3][q] = jrk0;
    L.d0[q] = kn.t0;
}

__device__ __forceinline__ void eval_query(const EvalLds &L, int q, double tau, double &pos, double &vel, double &acc)
{
    const double d0 = L.d0[q];
    const int seg = !(tau < d0);
    const double s = seg ? tau - d0 : tau;
    const double x0 = L.c[seg][0][q], va = L.c[seg][1][q], acc0 = L.c[seg][2][q], jrk0 = L.c[seg][3][q];
    pos = cubic_pos(x0, va, acc0, jrk0, s);
    vel = cubic_vel(va, acc0, jrk0, s);
    acc = cubic_acc(acc0, jrk0, s);
}

__device__ __forceinline__ void store_pair(double *out, size_t at, double a, double b, bool two)
{
    if (two) {
        const v2 both = {a, b};
        __builtin_nontemporal_store(both, reinterpret_cast<v2 *>(out + at));
    } else {
        out[at] = a;
    }
}

__device__ __forceinline__ void load_pair(const double *in, size_t at, bool two, double &a, double &b)
{
    if (two) {
        const v2 both = __builtin_nontemporal_load(reinterpret_cast<const v2 *>(in + at));
        a = both[0];
        b = both[1];
    } else {
        a = in[at];
        b = a;
    }
}

// a window's two ends, for a pair or a single query; a null array: the whole spline
__device__ __forceinline__ void load_window(const double *lo, const double *hi, size_t at, bool two, double &la, double &lb, double &ha, double &hb)
{
    const double inf = __builtin_inf();
    la = lb = -inf;
    ha = hb = inf;
    if (lo) load_pair(lo, at, two, la, lb);
    if (hi) load_pair(hi, at, two, ha, hb);
}

template <class Stage>
__device__ __forceinline__ void eval_trips(const Stage &stage, size_t n, size_t k, int P, const double *__restrict__ tau,
                                           double *__restrict__ pos, double *__restrict__ vel, double *__restrict__ acc)
{
    __shared__ EvalLds L;
    for_each_trip(n, P, [&](int q, size_t i) { stage_eval(L, q, stage.load(i)); }, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double ta, tb, pa, va, aa, pb, vb, ab;
            load_pair(tau, e_first + e, two, ta, tb);
            eval_query(L, qa, ta, pa, va, aa);
            eval_query(L, qb, tb, pb, vb, ab);
            if (pos) store_pair(pos, e_first + e, pa, pb, two);
            if (vel) store_pair(vel, e_first + e, va, vb, two);
            if (acc) store_pair(acc, e_first + e, aa, ab, two);
        });
    });
}

__global__ void __launch_bounds__(kTrajBlock)
k_trajectory_eval(FromArrays stage, size_t n, size_t k, int P, const double *__restrict__ tau, double *__restrict__ pos,
                  double *__restrict__ vel, double *__restrict__ acc)
{
    eval_trips(stage, n, k, P, tau, pos, vel, acc);
}

// the batch's current state, PROBLEM order: only the staging differs
template <typename S, int VARIANT, bool ZV>
__global__ void __launch_bounds__(kTrajBlock)
k_batch_trajectory(FromBatch<S, VARIANT, ZV> stage, size_t n, size_t k, int P, const double *__restrict__ tau, double *__restrict__ pos,
                   double *__restrict__ vel, double *__restrict__ acc)
{
    eval_trips(stage, n, k, P, tau, pos, vel, acc);
}

// ---- forward mode: tangents on the eight parameters and on tau in, tangents of pos, vel, acc out ----
struct JvpLds {
    double c[2][4][kTrajProblems];      // per segment: x0, va, acc0, jrk0 ...
    double t[2][4][kTrajProblems];      // ... and their tangents
    double d0[kTrajProblems], d0_dot[kTrajProblems];
};

// tangents of (acc0, jrk0): d(1/h) = -hd / h^2, d(1/h^2) = -2 hd / h^3
__device__ __forceinline__ void segment_tangents(double dx, double va, double vb, double acc0, double ih, double dxd, double vad, double vbd,
                                                 double hd, double &acc0d, double &jrk0d)
{
    const double ih2 = ih * ih, ih3 = ih2 * ih;
    acc0d = dxd * (6.0 * ih2) - dx * (12.0 * ih3) * hd - (vad * 4.0 + vbd * 2.0) * ih + (va * 4.0 + vb * 2.0) * ih2 * hd;
    jrk0d = (vbd - vad) * (2.0 * ih2) - (vb - va) * (4.0 * ih3) * hd - acc0d * (2.0 * ih) + acc0 * (2.0 * ih2) * hd;
}


// One problem's constants and their tangents along a direction, one segment at a time (a loop the compiler is told to keep): the
// sixteen loads of a problem and its tangents, taken at once, cost the registers of two waves per SIMD.  pos1, vel1 and their tangents
// are asked for in both passes (same thread, same address: the second is a cache hit).  store(seg, segment) puts a segment's numbers
// where the kernel keeps them; the durations and their tangents come back.
struct DirectedSegment { double x0, va, vb, dx, acc0, jrk0, ih, x0d, vad, vbd, dxd, acc0d, jrk0d, hd; };
struct DirectedDurations { double t0, t1, t0d, t1d; };

template <class Store> __device__ __forceinline__ DirectedDurations stage_directed(size_t i, const Spline8 &s, const Spline8 &dot, Store store)
{
    DirectedDurations d;
    d.t0 = s.p[6][i];
    d.t1 = s.p[7][i];
    check_durations(d.t0, d.t1);
    d.t0d = dot.p[6] ? dot.p[6][i] : 0.0;
    d.t1d = dot.p[7] ? dot.p[7][i] : 0.0;
#pragma nounroll
    for (int seg = 0; seg < 2; ++seg) {
        const double *pva = seg ? s.p[5] : s.p[3], *pvb = seg ? s.p[4] : s.p[5];      // vel0, vel1 | vel1, vel2
        const double *pvad = seg ? dot.p[5] : dot.p[3], *pvbd = seg ? dot.p[4] : dot.p[5];
        const double *px0 = seg ? s.p[1] : s.p[0], *px1 = seg ? s.p[2] : s.p[1];
        const double *px0d = seg ? dot.p[1] : dot.p[0], *px1d = seg ? dot.p[2] : dot.p[1];
        const double x0 = px0[i], x1 = px1[i], va = pva ? pva[i] : 0.0, vb = pvb ? pvb[i] : 0.0;
        const double x0d = px0d ? px0d[i] : 0.0, x1d = px1d ? px1d[i] : 0.0, vad = pvad ? pvad[i] : 0.0, vbd = pvbd ? pvbd[i] : 0.0;
        const double ih = rcp_<double>(seg ? d.t1 : d.t0), hd = seg ? d.t1d : d.t0d;
        const double dx = x1 - x0, dxd = x1d - x0d;
        double acc0, jrk0, acc0d, jrk0d;
        segment_constants(x0, x1, va, vb, ih, acc0, jrk0);
        segment_tangents(dx, va, vb, acc0, ih, dxd, vad, vbd, hd, acc0d, jrk0d);
        store(seg, DirectedSegment{x0, va, vb, dx, acc0, jrk0, ih, x0d, vad, vbd, dxd, acc0d, jrk0d, hd});
    }
    return d;
}

__device__ __forceinline__ DirectedDurations stage_tangents(JvpLds &L, int q, size_t i, const Spline8 &s, const Spline8 &dot)
{
    const DirectedDurations d = stage_directed(i, s, dot, [&](int seg, const DirectedSegment &g) {
        L.c[seg][0][q] = g.x0; L.c[seg][1][q] = g.va; L.c[seg][2][q] = g.acc0; L.c[seg][3][q] = g.jrk0;
        L.t[seg][0][q] = g.x0d; L.t[seg][1][q] = g.vad; L.t[seg][2][q] = g.acc0d; L.t[seg][3][q] = g.jrk0d;
    });
    L.d0[q] = d.t0;
    L.d0_dot[q] = d.t0d;
    return d;
}

__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(8)))      // 64 VGPRs: without the hint the allocator stops at 65
k_trajectory_jvp(FromArrays stage, Spline8 dot, size_t n, size_t k, int P, const double *__restrict__ tau, const double *__restrict__ tau_dot,
                 double *__restrict__ pos_dot, double *__restrict__ vel_dot, double *__restrict__ acc_dot)
{
    __shared__ JvpLds L;
    for_each_trip(n, P, [&](int q, size_t i) { stage_tangents(L, q, i, stage.s, dot); }, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        auto query = [&](int q, double ta, double td, double &pd, double &vd, double &ad) {
            const double d0 = L.d0[q];
            const int seg = !(ta < d0);
            const double s = seg ? ta - d0 : ta, sd = seg ? td - L.d0_dot[q] : td;
            const double va = L.c[seg][1][q], acc0 = L.c[seg][2][q], jrk0 = L.c[seg][3][q];
            const double x0d = L.t[seg][0][q], vad = L.t[seg][1][q], acc0d = L.t[seg][2][q], jrk0d = L.t[seg][3][q];
            const double vel = cubic_vel(va, acc0, jrk0, s), acc = cubic_acc(acc0, jrk0, s);
            pd = cubic_pos(x0d, vad, acc0d, jrk0d, s) + vel * sd;
            vd = cubic_vel(vad, acc0d, jrk0d, s) + acc * sd;
            ad = cubic_acc(acc0d, jrk0d, s) + jrk0 * sd;
        };
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double ta, tb, da = 0.0, db = 0.0, pa, va, aa, pb, vb, ab;
            load_pair(tau, e_first + e, two, ta, tb);
            if (tau_dot) load_pair(tau_dot, e_first + e, two, da, db);
            query(qa, ta, da, pa, va, aa);
            query(qb, tb, db, pb, vb, ab);
            if (pos_dot) store_pair(pos_dot, e_first + e, pa, pb, two);
            if (vel_dot) store_pair(vel_dot, e_first + e, va, vb, two);
            if (acc_dot) store_pair(acc_dot, e_first + e, aa, ab, two);
        });
    });
}

// ---- reverse mode ----
// With upstream gradients gp, gv, ga on pos, vel, acc and the sums restricted to the queries of a segment:
//     tau_bar = gp vel + gv acc + ga jrk0                                               (per query)
//     S_x = S gp    S_v = S (gp s + gv)    S_a = S (gp s^2 / 2 + gv s + ga)    S_j = S (gp s^3 / 6 + gv s^2 / 2 + ga s)
//     A = S_a - (2 / h) S_j
//     x0_bar = S_x - 6 A / h^2      x1_bar = 6 A / h^2
//     va_bar = S_v - 4 A / h - 2 S_j / h^2      vb_bar = -2 A / h + 2 S_j / h^2
//     h_bar = A (-12 (x1 - x0) / h^3 + (4 va + 2 vb) / h^2) + S_j (-4 (vb - va) / h^3 + 2 acc0 / h^2)
// Segment 0 sends them to (pos0, pos1, vel0, vel1, duration0), segment 1 to (pos1, pos2, vel1, vel2, duration1) and takes the sum
// of its queries' tau_bar off duration0_bar (s = tau - duration0 there).
struct VjpLds {
    double c[2][6][kTrajProblems];      // per segment: va, vb, x1 - x0, acc0, jrk0, 1 / h
    double d0[kTrajProblems];
    double bar[8][kTrajProblems];       // the problem's eight results, in the pointer table's order
};

struct SegmentBar { double x0, x1, va, vb, h; };

__device__ __forceinline__ SegmentBar segment_chain(const VjpLds &L, int seg, int q, double Sx, double Sv, double Sa, double Sj)
{
    const double va = L.c[seg][0][q], vb = L.c[seg][1][q], dx = L.c[seg][2][q], acc0 = L.c[seg][3][q], ih = L.c[seg][5][q];
    const double ih2 = ih * ih, ih3 = ih2 * ih;
    const double A = Sa - (2.0 * ih) * Sj;
    SegmentBar b;
    b.x1 = (6.0 * ih2) * A;
    b.x0 = Sx - b.x1;
    b.va = Sv - (4.0 * ih) * A - (2.0 * ih2) * Sj;
    b.vb = (2.0 * ih2) * Sj - (2.0 * ih) * A;
    b.h = A * ((va * 4.0 + vb * 2.0) * ih2 - dx * (12.0 * ih3)) + Sj * (acc0 * (2.0 * ih2) - (vb - va) * (4.0 * ih3));
    return b;
}

// one problem's constants for the reverse rule into LDS
__device__ __forceinline__ void stage_vjp(VjpLds &L, int q, Knots kn)
{
    kn.check();
    const double ih0 = rcp_<double>(kn.t0), ih1 = rcp_<double>(kn.t1);
    double acc0, jrk0;
    segment_constants(kn.p0, kn.p1, kn.v0, kn.v1, ih0, acc0, jrk0);
    L.c[0][0][q] = kn.v0; L.c[0][1][q] = kn.v1; L.c[0][2][q] = kn.p1 - kn.p0; L.c[0][3][q] = acc0; L.c[0][4][q] = jrk0; L.c[0][5][q] = ih0;
    segment_constants(kn.p1, kn.p2, kn.v1, kn.v2, ih1, acc0, jrk0);
    L.c[1][0][q] = kn.v1; L.c[1][1][q] = kn.v2; L.c[1][2][q] = kn.p2 - kn.p1; L.c[1][3][q] = acc0; L.c[1][4][q] = jrk0; L.c[1][5][q] = ih1;
    L.d0[q] = kn.t0;
}

// The reduction of the reverse rules: a group of G lanes per problem; row(q, at, two, sums) adds the pair of queries at element `at`
// (two) or the single one there to the lane's N sums, the lanes combine, and lane 0 gets finish(q, sums).  `two` is a literal in
// each of the two loops: a row body is compiled once for pairs and once for single elements.
// (The sums sit in a struct: a bare one-dimensional array the compiler turns into one wide vector register before it takes it apart,
// and k_vjp_integrals then carries some fifty register copies more per problem.)
template <int N> struct LaneSums { double s[N]; };

template <int N, class Row, class Finish>
__device__ __forceinline__ void reduce_rows(int G, int here, size_t p_first, size_t k, Row row, Finish finish)
{
    const int groups = kTrajBlock / G, group = (int)threadIdx.x / G, lane = (int)threadIdx.x & (G - 1);
    for (int q = group; q < here; q += groups) {
        const size_t first = (p_first + (size_t)q) * k;
        LaneSums<N> lane_sums = {};
        double (&sums)[N] = lane_sums.s;
        if ((k & 1) == 0) {      // k even: the row starts on a 16-byte boundary
            const size_t units = k >> 1;
            for (size_t u = lane; u < units; u += G) row(q, first + 2 * u, true, sums);
        } else {
            for (size_t u = lane; u < k; u += G) row(q, first + u, false, sums);
        }
        // the group's lanes combine: after the butterfly every lane holds the same N sums
        for (int m = 1; m < G; m <<= 1) {
#pragma unroll
            for (int i = 0; i < N; ++i) sums[i] += __shfl_xor(sums[i], m, 64);
        }
        if (lane == 0) finish(q, sums);
    }
}

// Segment 0's results go to (pos0, pos1, vel0, vel1), segment 1's to (pos1, pos2, vel1, vel2), in the pointer table's order; h0 and h1
// are the duration rows: the segments' own h and what the queries put on them.
__device__ __forceinline__ void route_bars(double (&bar)[8][kTrajProblems], int q, const SegmentBar &a, const SegmentBar &b, double h0, double h1)
{
    bar[0][q] = a.x0; bar[1][q] = a.x1 + b.x0; bar[2][q] = b.x1;
    bar[3][q] = a.va; bar[4][q] = b.vb; bar[5][q] = a.vb + b.va;
    bar[6][q] = h0; bar[7][q] = h1;
}

// once every group is through: the block's first `here` threads write their problem's wanted gradients
__device__ __forceinline__ void write_bars(const double (&bar)[8][kTrajProblems], const SplineBar8 &out, size_t p_first, int here)
{
    __syncthreads();
    if ((int)threadIdx.x < here) {
#pragma unroll
        for (int f = 0; f < 8; ++f)
            if (out.p[f]) out.p[f][p_first + threadIdx.x] = bar[f][threadIdx.x];
    }
}

// nine sums: S_x, S_v, S_a, S_j of segment 0, of segment 1, and the sum of tau_bar over segment 1
__global__ void __launch_bounds__(kTrajBlock)
k_trajectory_vjp(FromArrays stage, size_t n, size_t k, int P, int G, const double *__restrict__ tau, const double *__restrict__ g_pos,
                 const double *__restrict__ g_vel, const double *__restrict__ g_acc, SplineBar8 bar, double *__restrict__ tau_bar)
{
    __shared__ VjpLds L;
    for_each_trip(n, P, [&](int q, size_t i) { stage_vjp(L, q, stage.load(i)); }, [&](size_t p_first, int here) {
        auto query = [&](int q, double ta, double gp, double gv, double ga, double *S) -> double {
            const double d0 = L.d0[q];
            const bool seg = !(ta < d0);
            const double s = seg ? ta - d0 : ta;
            const double va = L.c[seg][0][q], acc0 = L.c[seg][3][q], jrk0 = L.c[seg][4][q];
            const double vel = cubic_vel(va, acc0, jrk0, s), acc = cubic_acc(acc0, jrk0, s);
            const double tb = gp * vel + gv * acc + ga * jrk0;
            const double h2 = s * (s * 0.5), h3 = h2 * (s * (1.0 / 3.0));
            const double w0 = gp, w1 = gp * s + gv, w2 = gp * h2 + gv * s + ga, w3 = gp * h3 + gv * h2 + ga * s;
            S[0] += seg ? 0.0 : w0; S[1] += seg ? 0.0 : w1; S[2] += seg ? 0.0 : w2; S[3] += seg ? 0.0 : w3;
            S[4] += seg ? w0 : 0.0; S[5] += seg ? w1 : 0.0; S[6] += seg ? w2 : 0.0; S[7] += seg ? w3 : 0.0;
            S[8] += seg ? tb : 0.0;
            return tb;
        };
        reduce_rows<9>(G, here, p_first, k, [&](int q, size_t at, bool two, double *S) {
            double ta, tb, pa = 0.0, pb = 0.0, va = 0.0, vb = 0.0, aa = 0.0, ab = 0.0;
            load_pair(tau, at, two, ta, tb);
            if (g_pos) load_pair(g_pos, at, two, pa, pb);
            if (g_vel) load_pair(g_vel, at, two, va, vb);
            if (g_acc) load_pair(g_acc, at, two, aa, ab);
            const double ba = query(q, ta, pa, va, aa, S);
            const double bb = two ? query(q, tb, pb, vb, ab, S) : ba;
            if (tau_bar) store_pair(tau_bar, at, ba, bb, two);
        }, [&](int q, const double *S) {
            const SegmentBar a = segment_chain(L, 0, q, S[0], S[1], S[2], S[3]);
            const SegmentBar b = segment_chain(L, 1, q, S[4], S[5], S[6], S[7]);
            route_bars(L.bar, q, a, b, a.h - S[8], b.h);
        });
        write_bars(L.bar, bar, p_first, here);
    });
}

// ---- second order: the derivative of the reverse rule along a direction (rp_trajectory_eval_hvp) ----
// With the upstream gradients held fixed and the direction (x0d, x1d, vad, vbd, hd) on the segment's ends, sd on its local time (tau_dot in
// segment 0, tau_dot - duration0_dot in segment 1) and (acc0d, jrk0d) from segment_tangents, the four weights w0 .. w3 of the reverse rule:
//     vel_d = vad + (acc0d + jrk0d s / 2) s + acc sd      acc_d = acc0d + jrk0d s + jrk0 sd
//     tau_bar_dot = gp vel_d + gv acc_d + ga jrk0d                                       (per query)
//     S_vd = S w0 sd    S_ad = S w1 sd    S_jd = S w2 sd      (S_x has no derivative)
//     A_d = S_ad - 2 S_jd / h + 2 S_j hd / h^2
//     x1_bar_dot = 6 A_d / h^2 - 12 A hd / h^3      x0_bar_dot = -x1_bar_dot
//     va_bar_dot = S_vd - 4 A_d / h + 4 A hd / h^2 - 2 S_jd / h^2 + 4 S_j hd / h^3
//     vb_bar_dot = -2 A_d / h + 2 A hd / h^2 + 2 S_jd / h^2 - 4 S_j hd / h^3
//     h_bar_dot = A_d c1 + A c1d + S_jd c2 + S_j c2d      (c1, c2 the two brackets of h_bar, c1d, c2d their derivatives)
// routed as the reverse rule's, duration0 taking off the sum of tau_bar_dot over segment 1.  reduce_rows over eleven sums: S_a and S_j
// of each segment (S_x and S_v are in no derivative: they enter the reverse rule linearly, with constant coefficients), the six dotted
// ones and that sum.
struct HvpLds {
    double c[2][6][kTrajProblems];      // per segment: va, vb, x1 - x0, acc0, jrk0, 1 / h ...
    double t[2][6][kTrajProblems];      // ... and along the direction: vad, vbd, x1d - x0d, acc0d, jrk0d, hd
    double d0[kTrajProblems], d0_dot[kTrajProblems];
    double bar[8][kTrajProblems];       // the problem's eight results, in the pointer table's order
};

// one problem's constants and their derivatives along the direction into LDS
__device__ __forceinline__ DirectedDurations stage_hvp(HvpLds &L, int q, size_t i, const Spline8 &s, const Spline8 &dot)
{
    const DirectedDurations d = stage_directed(i, s, dot, [&](int seg, const DirectedSegment &g) {
        L.c[seg][0][q] = g.va; L.c[seg][1][q] = g.vb; L.c[seg][2][q] = g.dx; L.c[seg][3][q] = g.acc0; L.c[seg][4][q] = g.jrk0; L.c[seg][5][q] = g.ih;
        L.t[seg][0][q] = g.vad; L.t[seg][1][q] = g.vbd; L.t[seg][2][q] = g.dxd; L.t[seg][3][q] = g.acc0d; L.t[seg][4][q] = g.jrk0d; L.t[seg][5][q] = g.hd;
    });
    L.d0[q] = d.t0;
    L.d0_dot[q] = d.t0d;
    return d;
}

// S: S_a, S_j of the segment; D: S_vd, S_ad, S_jd
__device__ __forceinline__ SegmentBar segment_chain_dot(const HvpLds &L, int seg, int q, const double *S, const double *D)
{
    const double va = L.c[seg][0][q], vb = L.c[seg][1][q], dx = L.c[seg][2][q], acc0 = L.c[seg][3][q], ih = L.c[seg][5][q];
    const double vad = L.t[seg][0][q], vbd = L.t[seg][1][q], dxd = L.t[seg][2][q], acc0d = L.t[seg][3][q], hd = L.t[seg][5][q];
    const double ih2 = ih * ih, ih3 = ih2 * ih, ih4 = ih2 * ih2;
    const double Sj = S[1], Svd = D[0], Sad = D[1], Sjd = D[2];
    const double A = S[0] - (2.0 * ih) * Sj;
    const double Ad = Sad - (2.0 * ih) * Sjd + ((2.0 * ih2) * Sj) * hd;
    SegmentBar b;
    b.x1 = (6.0 * ih2) * Ad - ((12.0 * ih3) * A) * hd;
    b.x0 = -b.x1;
    b.va = Svd - (4.0 * ih) * Ad + ((4.0 * ih2) * A) * hd - (2.0 * ih2) * Sjd + ((4.0 * ih3) * Sj) * hd;
    b.vb = (2.0 * ih2) * Sjd - (2.0 * ih) * Ad + ((2.0 * ih2) * A) * hd - ((4.0 * ih3) * Sj) * hd;
    const double c1 = (va * 4.0 + vb * 2.0) * ih2 - dx * (12.0 * ih3), c2 = acc0 * (2.0 * ih2) - (vb - va) * (4.0 * ih3);
    const double c1d = (vad * 4.0 + vbd * 2.0) * ih2 - dxd * (12.0 * ih3) + (dx * (36.0 * ih4) - (va * 4.0 + vb * 2.0) * (2.0 * ih3)) * hd;
    const double c2d = acc0d * (2.0 * ih2) - (vbd - vad) * (4.0 * ih3) + ((vb - va) * (12.0 * ih4) - acc0 * (4.0 * ih3)) * hd;
    b.h = Ad * c1 + A * c1d + Sjd * c2 + Sj * c2d;
    return b;
}

// eleven sums: S_a, S_j, S_vd, S_ad, S_jd of segment 0, of segment 1, and the sum of tau_bar_dot over segment 1
__global__ void __launch_bounds__(kTrajBlock)
k_trajectory_hvp(FromArrays stage, Spline8 dot, size_t n, size_t k, int P, int G, const double *__restrict__ tau, const double *__restrict__ g_pos,
                 const double *__restrict__ g_vel, const double *__restrict__ g_acc, const double *__restrict__ tau_dot, SplineBar8 bar,
                 double *__restrict__ tau_bar_dot)
{
    __shared__ HvpLds L;
    for_each_trip(n, P, [&](int q, size_t i) { stage_hvp(L, q, i, stage.s, dot); }, [&](size_t p_first, int here) {
        auto query = [&](int q, double ta, double td, double gp, double gv, double ga, double *S) -> double {
            const double d0 = L.d0[q], d0d = L.d0_dot[q];
            const bool seg = !(ta < d0);
            const double s = seg ? ta - d0 : ta, sd = seg ? td - d0d : td;
            const double acc0 = L.c[seg][3][q], jrk0 = L.c[seg][4][q];
            const double vad = L.t[seg][0][q], acc0d = L.t[seg][3][q], jrk0d = L.t[seg][4][q];
            const double acc = cubic_acc(acc0, jrk0, s);
            const double vel_d = cubic_vel(vad, acc0d, jrk0d, s) + acc * sd, acc_d = cubic_acc(acc0d, jrk0d, s) + jrk0 * sd;
            const double tbd = gp * vel_d + gv * acc_d + ga * jrk0d;
            const double h2 = s * (s * 0.5), h3 = h2 * (s * (1.0 / 3.0));
            const double w0 = gp, w1 = gp * s + gv, w2 = gp * h2 + gv * s + ga, w3 = gp * h3 + gv * h2 + ga * s;
            const double u0 = w0 * sd, u1 = w1 * sd, u2 = w2 * sd;
            S[0] += seg ? 0.0 : w2; S[1] += seg ? 0.0 : w3;
            S[5] += seg ? w2 : 0.0; S[6] += seg ? w3 : 0.0;
            S[2] += seg ? 0.0 : u0; S[3] += seg ? 0.0 : u1; S[4] += seg ? 0.0 : u2;
            S[7] += seg ? u0 : 0.0; S[8] += seg ? u1 : 0.0; S[9] += seg ? u2 : 0.0;
            S[10] += seg ? tbd : 0.0;
            return tbd;
        };
        reduce_rows<11>(G, here, p_first, k, [&](int q, size_t at, bool two, double *S) {
            double ta, tb, da = 0.0, db = 0.0, pa = 0.0, pb = 0.0, va = 0.0, vb = 0.0, aa = 0.0, ab = 0.0;
            load_pair(tau, at, two, ta, tb);
            if (tau_dot) load_pair(tau_dot, at, two, da, db);
            if (g_pos) load_pair(g_pos, at, two, pa, pb);
            if (g_vel) load_pair(g_vel, at, two, va, vb);
            if (g_acc) load_pair(g_acc, at, two, aa, ab);
            const double ba = query(q, ta, da, pa, va, aa, S);
            const double bb = two ? query(q, tb, db, pb, vb, ab, S) : ba;
            if (tau_bar_dot) store_pair(tau_bar_dot, at, ba, bb, two);
        }, [&](int q, const double *S) {
            const SegmentBar a = segment_chain_dot(L, 0, q, S, S + 2);
            const SegmentBar b = segment_chain_dot(L, 1, q, S + 5, S + 7);
            route_bars(L.bar, q, a, b, a.h - S[10], b.h);
        });
        write_bars(L.bar, bar, p_first, here);
    });
}

// ---- the inverse question: when does the spline first reach a level (rp_trajectory_crossing, rp_batch_crossing_device) ----
// In a segment the velocity va + acc0 s + (jrk0 / 2) s^2 has at most two roots strictly inside (0, h): they cut the segment into at most
// three monotone pieces, padded to exactly three with breakpoints 0 <= c1 <= c2 <= h (a missing smaller root: c1 = 0, a missing larger
// one: c2 = h; a piece of length zero is harmless).  The block's first P threads leave per problem, next to the evaluator's constants, the
// four inner breakpoints, duration1 and pos at the seven piece ends (pos1 itself at the knot, as the evaluator gives it at tau =
// duration0).  A query walks the six pieces in time order, takes the first whose end positions hold its level between them, and solves
// pos(s) = level inside that bracket by Newton steps kept inside it (bisection where a step leaves the bracket or fails to halve the step
// before last), in eval_query's arithmetic, until g == 0, the bracket or the step is within 2 ulp of the piece's later end, or a Newton step's
// own error estimate is; the answer is the point of smallest |g| among those looked at.  The loop's trip bound is a compile-time constant:
// no input can make it spin.
constexpr int kCrossTrips = 64;                        // bisection alone reaches 2 ulp of any double bracket in ~53
constexpr double kCrossTol = 2.0 * 2.220446049250313e-16;      // the stopping width, as a fraction of the piece's later end: 2 ulp

struct CrossLds {
    EvalLds e;
    double brk[2][2][kTrajProblems];      // per segment: c1, c2
    double d1[kTrajProblems];
    double end[7][kTrajProblems];         // pos at 0, c1, c2 of segment 0, at the knot, at c1, c2, duration1 of segment 1
};

// the roots of one segment's velocity, by the quadratic formula that does not cancel: q = -(b + sgn(b) sqrt(disc)) / 2, roots q / a and
// c / q (NaN: no such root)
__device__ __forceinline__ void velocity_roots(double va, double acc0, double jrk0, double &r0, double &r1)
{
    const double a = jrk0 * 0.5, b = acc0, c = va;
    const double disc = b * b - 4.0 * (a * c);
    r0 = r1 = quiet_nan();
    if (disc >= 0.0) {      // a NaN fails
        const double q = -0.5 * (b + __builtin_copysign(sqrt_<double>(disc), b));
        if (a != 0.0) r0 = q / a;
        r1 = c / q;      // q == 0: inf or NaN, not inside
    }
}

// the breakpoints of one segment
__device__ __forceinline__ void velocity_breaks(double va, double acc0, double jrk0, double h, double &c1, double &c2)
{
    double r0, r1;
    velocity_roots(va, acc0, jrk0, r0, r1);
    const bool in0 = r0 > 0.0 && r0 < h, in1 = r1 > 0.0 && r1 < h;      // strictly inside: a rest start's root at s = 0 is not
    c1 = 0.0;
    c2 = h;
    if (in0 && in1) {
        c1 = r0 < r1 ? r0 : r1;
        c2 = r0 < r1 ? r1 : r0;
    } else if (in0 || in1) {
        const double r = in0 ? r0 : r1, other = in0 ? r1 : r0;
        if (other <= 0.0) c2 = r; else c1 = r;      // the one inside is the larger root | the smaller (or the only) one
    }
}

__device__ __forceinline__ double pos_at(const EvalLds &L, int seg, int q, double s)
{
    return cubic_pos(L.c[seg][0][q], L.c[seg][1][q], L.c[seg][2][q], L.c[seg][3][q], s);
}

// both segments' breakpoints from constants already staged: va, acc0, jrk0 are the rows of c that hold them; each(seg, h, c1, c2) for
// what else a kernel keeps per segment
template <int ROWS, class Each>
__device__ __forceinline__ void stage_breaks(double (&brk)[2][2][kTrajProblems], int q, const double (&c)[2][ROWS][kTrajProblems], int va, int acc0,
                                             int jrk0, double t0, double t1, Each each)
{
#pragma unroll
    for (int seg = 0; seg < 2; ++seg) {
        const double h = seg ? t1 : t0;
        double c1, c2;
        velocity_breaks(c[seg][va][q], c[seg][acc0][q], c[seg][jrk0][q], h, c1, c2);
        brk[seg][0][q] = c1;
        brk[seg][1][q] = c2;
        each(seg, h, c1, c2);
    }
}

template <int ROWS>
__device__ __forceinline__ void stage_breaks(double (&brk)[2][2][kTrajProblems], int q, const double (&c)[2][ROWS][kTrajProblems], int va, int acc0,
                                             int jrk0, double t0, double t1)
{
    stage_breaks(brk, q, c, va, acc0, jrk0, t0, t1, [](int, double, double, double) {});
}

__device__ __forceinline__ void stage_crossing(CrossLds &L, int q, Knots kn)
{
    kn.check();
    stage_eval(L.e, q, kn);
    L.d1[q] = kn.t1;
    stage_breaks(L.brk, q, L.e.c, 1, 2, 3, kn.t0, kn.t1, [&](int seg, double h, double c1, double c2) {
        L.end[3 * seg][q] = pos_at(L.e, seg, q, 0.0);      // x0, or NaN with the problem's constants
        L.end[3 * seg + 1][q] = pos_at(L.e, seg, q, c1);
        L.end[3 * seg + 2][q] = pos_at(L.e, seg, q, c2);
        if (seg) L.end[6][q] = pos_at(L.e, 1, q, h);
    });
}

// The search both inverse questions share (crossing_query, meeting_query): the root of cubic_pos(x0, va, acc0, jrk0, s) - p in the bracket
// [lo, hi] of one monotone piece, whose ends leave g_lo != 0 and g_hi; tol is the stopping width.  The point of smallest |g| looked at.
__device__ __forceinline__ double bracket_search(double x0, double va, double acc0, double jrk0, double p, double lo, double hi, double g_lo,
                                                 double g_hi, double tol)
{
    const bool up = g_lo < 0.0;
    double width = hi - lo;
    double best = abs_(g_hi) < abs_(g_lo) ? hi : lo, best_g = min_(abs_(g_lo), abs_(g_hi));      // the smallest |g| seen, and where
    double s = lo + width * (g_lo * rcp_<double>(g_lo - g_hi));      // the secant point of the bracket
    if (!(s > lo && s < hi)) s = lo + 0.5 * width;
    double dx_old = width, dx = width;
    bool last = false;
    for (int trip = 0; trip < kCrossTrips; ++trip) {
        const double g = cubic_pos(x0, va, acc0, jrk0, s) - p;
        const double v = cubic_vel(va, acc0, jrk0, s);
        if (abs_(g) < best_g) { best_g = abs_(g); best = s; }
        if (g == 0.0 || last) break;
        if ((g < 0.0) == up) lo = s; else hi = s;
        width = hi - lo;
        if (!(width > tol)) break;
        const double step = g * rcp_<double>(v);      // v == 0: infinite, outside
        double next = s - step;
        const bool newton = next > lo && next < hi && 2.0 * abs_(step) <= abs_(dx_old);
        if (!newton) next = lo + 0.5 * width;
        // a Newton step leaves an error of about |acc / (2 vel)| step^2: once that is below the stopping width, the point it leads to is
        // the last one looked at (further steps would only follow the rounding of g around)
        last = newton && abs_(cubic_acc(acc0, jrk0, s)) * (step * step) <= (2.0 * tol) * abs_(v);
        dx_old = dx;
        dx = next - s;
        if (!(abs_(dx) > tol)) break;
        s = next;
    }
    return best;
}

__device__ __forceinline__ void crossing_query(const CrossLds &L, int q, double p, double &time, double &vel)
{
    // the first piece, in time order, whose end positions hold p between them (a NaN or infinite p, NaN ends: none)
    int m = -1;
    double p_lo = 0.0, p_hi = 0.0, later = L.end[6][q];
#pragma unroll
    for (int j = 5; j >= 0; --j) {
        const double sooner = L.end[j][q];
        if ((sooner <= p && p <= later) || (later <= p && p <= sooner)) { m = j; p_lo = sooner; p_hi = later; }
        later = sooner;
    }
    time = vel = quiet_nan();
    if (m < 0) return;
    const int seg = m >= 3, j = m - 3 * seg;
    const double lo = j == 0 ? 0.0 : L.brk[seg][j - 1][q];
    const double hi = j == 2 ? (seg ? L.d1[q] : L.e.d0[q]) : L.brk[seg][j][q];
    const double x0 = L.e.c[seg][0][q], va = L.e.c[seg][1][q], acc0 = L.e.c[seg][2][q], jrk0 = L.e.c[seg][3][q];
    const double g_lo = p_lo - p, g_hi = p_hi - p;
    double s = lo;      // g_lo == 0: the breakpoint itself (p == pos0: tau = 0 exactly)
    if (g_lo != 0.0) s = bracket_search(x0, va, acc0, jrk0, p, lo, hi, g_lo, g_hi, kCrossTol * hi);
    time = seg ? L.e.d0[q] + s : s;
    vel = cubic_vel(va, acc0, jrk0, s);
}

template <class Stage>
__device__ __forceinline__ void crossing_trips(const Stage &stage, size_t n, size_t k, int P, const double *__restrict__ level,
                                               double *__restrict__ time, double *__restrict__ vel)
{
    __shared__ CrossLds L;
    // (the two query lambdas hold copies, not references: with references the compiler leaves a few more address-space checks of the LDS
    // pointers that crossing_query selects among)
    for_each_trip(n, P, [&](int q, size_t i) { stage_crossing(L, q, stage.load(i)); }, [=](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        stream_pairs(here, k, [=](size_t e, int qa, int qb, bool two) {
            double pa, pb, ta, tb, va, vb;
            load_pair(level, e_first + e, two, pa, pb);
            crossing_query(L, qa, pa, ta, va);
            if (two) crossing_query(L, qb, pb, tb, vb); else { tb = ta; vb = va; }
            store_pair(time, e_first + e, ta, tb, two);
            if (vel) store_pair(vel, e_first + e, va, vb, two);
        });
    });
}

__global__ void __launch_bounds__(kTrajBlock)
k_crossing(FromArrays stage, size_t n, size_t k, int P, const double *__restrict__ level, double *__restrict__ time, double *__restrict__ vel)
{
    crossing_trips(stage, n, k, P, level, time, vel);
}

template <typename S, int VARIANT, bool ZV>
__global__ void __launch_bounds__(kTrajBlock)
k_batch_crossing(FromBatch<S, VARIANT, ZV> stage, size_t n, size_t k, int P, const double *__restrict__ level, double *__restrict__ time,
                 double *__restrict__ vel)
{
    crossing_trips(stage, n, k, P, level, time, vel);
}
// a query's window [lo, hi], clamped to [0, T]
struct Window {
    double a, b;
    bool ok, lo_taken, hi_taken;      // a <= b; a is lo (not the clamp +0.0); b is hi (not the clamp T)
};

__device__ __forceinline__ Window clamp_window(double lo, double hi, double T)
{
    Window w;
    w.lo_taken = lo > 0.0;
    w.hi_taken = hi < T;
    w.a = w.lo_taken ? lo : (lo != lo ? lo : 0.0);      // a NaN end stays one
    w.b = w.hi_taken ? hi : (hi != hi ? hi : T);
    w.ok = w.a <= w.b;      // a NaN end, a NaN T, a window outside [0, T]: nothing
    return w;
}

// ---- how far and how fast at most: the extreme position and velocity over a window (rp_trajectory_extrema, rp_batch_extrema_device;
// DESIGN.md section 15) ----
// On a window [a, b] inside [0, T] the extreme of pos is at a, at b, at the knot, or at a root of a segment's velocity strictly inside
// (0, h); that of vel at a, at b, at the knot, or at a segment's s = -acc0 / jrk0 strictly inside (0, h).  The block's first P threads
// leave per problem, next to the evaluator's constants, those six stationary times as global times (NaN: none; the smaller root of a
// segment first), pos or vel there through eval_query at that global time, and T = duration0 + duration1.  A query clamps its window,
// evaluates a, the knot and b, and walks the candidates in time order keeping the strictly better one: the earliest among equals, a NaN
// never.  No search and no loop: selects only.  The time that comes back carries its candidate's own bits (lo or +0.0, hi or T,
// duration0, the staged time) -- the torch layer tells the candidates apart by equality -- and the value is eval_query's at that time.
struct ExtLds {
    EvalLds e;
    double tp[4][kTrajProblems];      // the roots of vel, global: two of segment 0, two of segment 1
    double pp[4][kTrajProblems];      // pos there
    double tv[2][kTrajProblems];      // the root of acc, global: segment 0, segment 1
    double vv[2][kTrajProblems];      // vel there
    double T[kTrajProblems];
};

__device__ __forceinline__ void stage_extrema(ExtLds &L, int q, Knots kn)
{
    kn.check();
    stage_eval(L.e, q, kn);
    L.T[q] = kn.t0 + kn.t1;
#pragma unroll
    for (int seg = 0; seg < 2; ++seg) {
        const double h = seg ? kn.t1 : kn.t0, off = seg ? kn.t0 : 0.0;
        const double va = L.e.c[seg][1][q], acc0 = L.e.c[seg][2][q], jrk0 = L.e.c[seg][3][q];
        double r0, r1;
        velocity_roots(va, acc0, jrk0, r0, r1);
        if (!(r0 > 0.0 && r0 < h)) r0 = quiet_nan();
        if (!(r1 > 0.0 && r1 < h)) r1 = quiet_nan();
        const bool swap = r1 < r0 || r0 != r0;      // time order; a lone root comes first
        const double first = swap ? r1 : r0, second = swap ? r0 : r1;
        double s = jrk0 != 0.0 ? -acc0 / jrk0 : quiet_nan();
        if (!(s > 0.0 && s < h)) s = quiet_nan();      // an infinite or NaN quotient is not inside
        const double t[3] = {off + first, off + second, off + s};
        double pos, vel, acc;
        eval_query(L.e, q, t[0], pos, vel, acc);
        L.tp[2 * seg][q] = t[0]; L.pp[2 * seg][q] = pos;
        eval_query(L.e, q, t[1], pos, vel, acc);
        L.tp[2 * seg + 1][q] = t[1]; L.pp[2 * seg + 1][q] = pos;
        eval_query(L.e, q, t[2], pos, vel, acc);
        L.tv[seg][q] = t[2]; L.vv[seg][q] = vel;
    }
}

// the running extremes of one quantity: a candidate replaces the minimum (maximum) only where it is strictly smaller (larger), or where
// nothing has been taken yet; a NaN value never compares
struct Extreme {
    double lo_v, lo_t, hi_v, hi_t;
    __device__ __forceinline__ void take(bool ok, double t, double v)
    {
        const bool less = ok && (v < lo_v || (lo_v != lo_v && v == v)), more = ok && (v > hi_v || (hi_v != hi_v && v == v));
        lo_v = less ? v : lo_v; lo_t = less ? t : lo_t;
        hi_v = more ? v : hi_v; hi_t = more ? t : hi_t;
    }
};

template <bool POS, bool VEL>
__device__ __forceinline__ void extrema_query(const ExtLds &L, int q, double lo, double hi, Extreme &P, Extreme &V)
{
    const double nan = quiet_nan();
    P = Extreme{nan, nan, nan, nan};
    V = Extreme{nan, nan, nan, nan};
    const double d0 = L.e.d0[q];
    const Window win = clamp_window(lo, hi, L.T[q]);
    const double a = win.a, b = win.b;
    const bool ok = win.ok;      // not: no candidate at all
    double pa, va, pk, vk, pb, vb, acc;
    eval_query(L.e, q, a, pa, va, acc);
    eval_query(L.e, q, d0, pk, vk, acc);
    eval_query(L.e, q, b, pb, vb, acc);
    const bool knot = ok && a <= d0 && d0 <= b;
    if (POS) {
        P.take(ok, a, pa);
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            if (c == 2) P.take(knot, d0, pk);
            const double t = L.tp[c][q];
            P.take(ok && a < t && t < b, t, L.pp[c][q]);
        }
        P.take(ok, b, pb);
    }
    if (VEL) {
        V.take(ok, a, va);
        const double t0 = L.tv[0][q], t1 = L.tv[1][q];
        V.take(ok && a < t0 && t0 < b, t0, L.vv[0][q]);
        V.take(knot, d0, vk);
        V.take(ok && a < t1 && t1 < b, t1, L.vv[1][q]);
        V.take(ok, b, vb);
    }
}

template <bool POS, bool VEL>
__device__ __forceinline__ void extrema_stream(const ExtLds &L, int here, size_t k, size_t e_first, const double *__restrict__ lo,
                                               const double *__restrict__ hi, const Out4 &value, const Out4 &time)
{
    stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
        double la, lb, ha, hb;
        load_window(lo, hi, e_first + e, two, la, lb, ha, hb);
        Extreme Pa, Va, Pb, Vb;
        extrema_query<POS, VEL>(L, qa, la, ha, Pa, Va);
        extrema_query<POS, VEL>(L, qb, lb, hb, Pb, Vb);
        if (POS) {
            if (value.p[0]) store_pair(value.p[0], e_first + e, Pa.lo_v, Pb.lo_v, two);
            if (value.p[1]) store_pair(value.p[1], e_first + e, Pa.hi_v, Pb.hi_v, two);
            if (time.p[0]) store_pair(time.p[0], e_first + e, Pa.lo_t, Pb.lo_t, two);
            if (time.p[1]) store_pair(time.p[1], e_first + e, Pa.hi_t, Pb.hi_t, two);
        }
        if (VEL) {
            if (value.p[2]) store_pair(value.p[2], e_first + e, Va.lo_v, Vb.lo_v, two);
            if (value.p[3]) store_pair(value.p[3], e_first + e, Va.hi_v, Vb.hi_v, two);
            if (time.p[2]) store_pair(time.p[2], e_first + e, Va.lo_t, Vb.lo_t, two);
            if (time.p[3]) store_pair(time.p[3], e_first + e, Va.hi_t, Vb.hi_t, two);
        }
    });
}

template <class Stage>
__device__ __forceinline__ void extrema_trips(const Stage &stage, size_t n, size_t k, int P, const double *__restrict__ lo,
                                              const double *__restrict__ hi, const Out4 &value, const Out4 &time)
{
    __shared__ ExtLds L;
    const bool pos = value.p[0] || value.p[1] || time.p[0] || time.p[1], vel = value.p[2] || value.p[3] || time.p[2] || time.p[3];      // uniform
    for_each_trip(n, P, [&](int q, size_t i) { stage_extrema(L, q, stage.load(i)); }, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        // the half nobody asked for is not computed (a speed limit wants vel alone)
        if (pos && vel) extrema_stream<true, true>(L, here, k, e_first, lo, hi, value, time);
        else if (pos) extrema_stream<true, false>(L, here, k, e_first, lo, hi, value, time);
        else extrema_stream<false, true>(L, here, k, e_first, lo, hi, value, time);
    });
}

__global__ void __launch_bounds__(kTrajBlock)
k_extrema(FromArrays stage, size_t n, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi, Out4 value, Out4 time)
{
    extrema_trips(stage, n, k, P, lo, hi, value, time);
}

template <typename S, int VARIANT, bool ZV>
__global__ void __launch_bounds__(kTrajBlock)
k_batch_extrema(FromBatch<S, VARIANT, ZV> stage, size_t n, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi,
                Out4 value, Out4 time)
{
    extrema_trips(stage, n, k, P, lo, hi, value, time);
}
// ---- how much: the integrals of pos, |vel|, vel^2 and acc^2 over a window (rp_trajectory_integrals, _vjp, _jvp, rp_batch_integrals_device;
// DESIGN.md section 16) ----
// The window is clamped as the extrema's, [a, b] inside [0, T], and split at the knot: segment 0 contributes over the local piece that
// starts at a and is min(b, duration0) - a long (if a < duration0), segment 1 over the one that starts at max(a, duration0) - duration0 and
// is b - max(a, duration0) long (if b > duration0).  Every integral is a polynomial in the piece's length w -- taken from the GLOBAL ends, so
// that it carries the rounding of b - a and not of the segment -- with coefficients from (X, V, A), the evaluator's pos, vel, acc at the
// piece's local start, and J = jrk0: no antiderivative is differenced, so a short window late in a segment keeps its digits.  The distance
// walks the segment's three monotone pieces (velocity_breaks) clipped to the window and adds |pos increment| of each, in the same shifted
// form from each piece's own start; a piece that holds the whole window has the window's own length w.  The block's first P threads leave per
// problem the evaluator's constants, the four inner breakpoints and T; selects only, no loop whose trip count depends on data.
// The derivatives: for one segment's contribution I(x0, va, acc0, jrk0; sa, sb), dI/dsb = f(sb), dI/dsa = -f(sa) with f the integrand, and
// the partials in the four constants are moments of the piece, again in the shifted form (segment_partials).  Reverse mode adds them, weighted
// by the upstream gradients, to k_trajectory_vjp's four sums per segment, in its order of additions, and the end terms to two more sums for
// the durations; forward mode contracts them with segment_tangents' tangents.  The end terms go where the end came from: a = lo -> lo;
// a = +0.0 -> nowhere; b = hi -> hi; b = T -> duration1 (as a local time of segment 1 the end is T - duration0 = duration1); segment 0's end
// on the knot -> duration0; a segment-1 end that is lo or hi -> also duration0, negated (its local time is the end - duration0).
struct IntLds {
    EvalLds e;
    double brk[2][2][kTrajProblems];      // per segment: c1, c2
    double T[kTrajProblems];
};

// a segment's constants and inner breakpoints, wherever the kernel keeps them
struct SegmentConst { double x0, va, acc0, jrk0, c1, c2; };

// the piece of the window in one segment: its local start and its length (both 0 where the segment does not contribute)
struct Piece {
    bool on;
    double sa, w;
};

__device__ __forceinline__ Piece segment_piece(int seg, const Window &win, double d0)
{
    Piece p;
    if (seg == 0) {
        p.on = win.ok && win.a < d0;
        p.sa = win.a;
        p.w = (win.b < d0 ? win.b : d0) - win.a;
    } else {
        p.on = win.ok && win.b > d0;
        const double start = win.a > d0 ? win.a : d0;
        p.sa = start - d0;
        p.w = win.b - start;
    }
    p.sa = p.on ? p.sa : 0.0;
    p.w = p.on ? p.w : 0.0;
    return p;
}

__device__ __forceinline__ void local_state(const SegmentConst &c, double s, double &X, double &V, double &A)
{
    X = cubic_pos(c.x0, c.va, c.acc0, c.jrk0, s);
    V = cubic_vel(c.va, c.acc0, c.jrk0, s);
    A = cubic_acc(c.acc0, c.jrk0, s);
}

// the three monotone pieces [0, c1], [c1, c2], [c2, ...) clipped to [sa, sa + w]: each(u, l, inc) gets the clipped piece's local start,
// its length (0: not in the window) and the pos increment over it.  The last piece has no end of its own: the window is inside the segment.
// UNROLLED: the three side by side (the forward), or a loop the compiler is told to keep (the derivatives, for their registers)
template <bool UNROLLED, class Each> __device__ __forceinline__ void monotone_pieces(const SegmentConst &c, const Piece &p, Each each)
{
    const double se = p.sa + p.w;
    auto piece = [&](int j) {
        const double pl = j == 0 ? 0.0 : (j == 1 ? c.c1 : c.c2), ph = j == 0 ? c.c1 : c.c2;
        const bool starts = p.sa >= pl, ends = j == 2 || se <= ph;
        const double u = starts ? p.sa : pl, e = ends ? se : ph;
        double l = starts && ends ? p.w : e - u;      // the window's own length where the piece holds all of it
        l = l > 0.0 ? l : 0.0;
        const double Vu = cubic_vel(c.va, c.acc0, c.jrk0, u), Au = cubic_acc(c.acc0, c.jrk0, u);
        each(u, l, l * (Vu + (l * 0.5) * (Au + (l * (1.0 / 3.0)) * c.jrk0)));
    };
    if (UNROLLED) {
        piece(0);
        piece(1);
        piece(2);
    } else {
#pragma nounroll
        for (int j = 0; j < 3; ++j) piece(j);
    }
}

// one segment's contributions to the four integrals
template <bool DIST> __device__ __forceinline__ void segment_values(const SegmentConst &c, const Piece &p, double v[4])
{
    const double w = p.w, J = c.jrk0;
    double X, V, A;
    local_state(c, p.sa, X, V, A);
    v[0] = w * (X + (w * 0.5) * (V + (w * (1.0 / 3.0)) * (A + (w * 0.25) * J)));
    v[2] = w * (V * V + w * (V * A + (w * (1.0 / 3.0)) * ((A * A + V * J) + w * (0.75 * (A * J) + (0.15 * w) * (J * J)))));
    v[3] = w * (A * A + w * (A * J + (w * (1.0 / 3.0)) * (J * J)));
    double dist = 0.0 * w;
    if (DIST) monotone_pieces<true>(c, p, [&](double, double, double inc) { dist += abs_(inc); });
    v[1] = dist;
}

__device__ __forceinline__ SegmentConst segment_const(const EvalLds &e, const double (&brk)[2][2][kTrajProblems], int seg, int q)
{
    return SegmentConst{e.c[seg][0][q], e.c[seg][1][q], e.c[seg][2][q], e.c[seg][3][q], brk[seg][0][q], brk[seg][1][q]};
}

__device__ __forceinline__ void stage_integrals(IntLds &L, int q, Knots kn)
{
    kn.check();
    stage_eval(L.e, q, kn);
    L.T[q] = kn.t0 + kn.t1;
    stage_breaks(L.brk, q, L.e.c, 1, 2, 3, kn.t0, kn.t1);
}

template <bool DIST> __device__ __forceinline__ void integrals_query(const IntLds &L, int q, double lo, double hi, double out[4])
{
    const double d0 = L.e.d0[q];
    const Window win = clamp_window(lo, hi, L.T[q]);
    double v0[4], v1[4];
    segment_values<DIST>(segment_const(L.e, L.brk, 0, q), segment_piece(0, win, d0), v0);
    segment_values<DIST>(segment_const(L.e, L.brk, 1, q), segment_piece(1, win, d0), v1);
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = win.ok ? (win.a == win.b ? 0.0 : v0[i] + v1[i]) : quiet_nan();
}

template <bool DIST>
__device__ __forceinline__ void integrals_stream(const IntLds &L, int here, size_t k, size_t e_first, const double *__restrict__ lo,
                                                 const double *__restrict__ hi, const Out4 &value)
{
    stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
        double la, lb, ha, hb, a[4], b[4];
        load_window(lo, hi, e_first + e, two, la, lb, ha, hb);
        integrals_query<DIST>(L, qa, la, ha, a);
        integrals_query<DIST>(L, qb, lb, hb, b);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (value.p[i]) store_pair(value.p[i], e_first + e, a[i], b[i], two);      // without DIST value.p[1] is null
    });
}

template <class Stage>
__device__ __forceinline__ void integrals_trips(const Stage &stage, size_t n, size_t k, int P, const double *__restrict__ lo,
                                                const double *__restrict__ hi, const Out4 &value)
{
    __shared__ IntLds L;
    const bool dist = value.p[1] != nullptr;      // uniform
    for_each_trip(n, P, [&](int q, size_t i) { stage_integrals(L, q, stage.load(i)); }, [&](size_t p_first, int here) {
        // the walk over the monotone pieces is most of the work: not taken where nobody asked for the distance
        if (dist) integrals_stream<true>(L, here, k, p_first * k, lo, hi, value);
        else integrals_stream<false>(L, here, k, p_first * k, lo, hi, value);
    });
}

__global__ void __launch_bounds__(kTrajBlock)
k_integrals(FromArrays stage, size_t n, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi, Out4 value)
{
    integrals_trips(stage, n, k, P, lo, hi, value);
}

template <typename S, int VARIANT, bool ZV>
__global__ void __launch_bounds__(kTrajBlock)
k_batch_integrals(FromBatch<S, VARIANT, ZV> stage, size_t n, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi,
                  Out4 value)
{
    integrals_trips(stage, n, k, P, lo, hi, value);
}

// The partials of one segment's contributions in (x0, va, acc0, jrk0) -- pos_int's four, the distance's, vel_sq's (none in x0) and acc_sq's
// (none in x0, va) -- and the four integrands at the piece's start and end.  With s = sa + t on the piece and vel = V + A t + J t^2 / 2:
//     pos_int   (w, M1, M2 / 2, M3 / 6)                              Mm = the integral of s^m
//     distance  the signed sums over its monotone pieces of (l, the integral of s, of s^2 / 2); a root inside contributes nothing, |vel| is 0 there
//     vel_sq    (2 Q0, 2 (sa Q0 + Q1), sa^2 Q0 + 2 sa Q1 + Q2)      Qm = the integral of vel t^m
//     acc_sq    (2 R0, 2 (sa R0 + R1))                               Rm = the integral of acc t^m
// each(i, m0, m1, m2, m3, fa, fb) gets output i's four partials and its integrand at the two ends, one output at a time and in the outputs'
// order, so that no more than one output's numbers are live.  Without DIST the walk over the monotone pieces is not made and the distance's
// partials are zeros (for a caller whose gradient on the distance is zero)
template <bool DIST = true, class Each> __device__ __forceinline__ void segment_partials(const SegmentConst &c, const Piece &p, Each each)
{
    const double w = p.w, sa = p.sa, J = c.jrk0, third = 1.0 / 3.0;
    double X, V, A;
    local_state(c, sa, X, V, A);
    const double Vb = V + w * (A + (w * 0.5) * J), Ab = A + w * J;
    {
        const double Xb = X + w * (V + (w * 0.5) * (A + (w * third) * J));
        const double M1 = w * (sa + w * 0.5), M2 = w * (sa * sa + w * (sa + w * third));
        const double M3 = w * (sa * sa * sa + w * (1.5 * (sa * sa) + w * (sa + w * 0.25)));
        each(0, w, M1, M2 * 0.5, M3 * (1.0 / 6.0), X, Xb);
    }
    {
        double d1 = 0.0 * w, d2 = d1, d3 = d1;
        if (DIST) monotone_pieces<false>(c, p, [&](double u, double l, double inc) {
            const double sign = inc > 0.0 ? 1.0 : (inc < 0.0 ? -1.0 : 0.0);
            d1 += sign * l;
            d2 += sign * (l * (u + l * 0.5));
            d3 += sign * (0.5 * (l * (u * u + l * (u + l * third))));
        });
        each(1, 0.0, d1, d2, d3, abs_(V), abs_(Vb));
    }
    {
        const double Q0 = w * (V + (w * 0.5) * (A + (w * third) * J));
        const double Q1 = (w * w) * (V * 0.5 + w * (A * third + (w * 0.125) * J));
        const double Q2 = (w * w * w) * (V * third + w * (A * 0.25 + (w * 0.1) * J));
        each(2, 0.0, 2.0 * Q0, 2.0 * (sa * Q0 + Q1), (sa * sa) * Q0 + (2.0 * sa) * Q1 + Q2, V * V, Vb * Vb);
    }
    {
        const double R0 = w * (A + (w * 0.5) * J), R1 = (w * w) * (A * 0.5 + (w * third) * J);
        each(3, 0.0, 0.0, 2.0 * R0, 2.0 * (sa * R0 + R1), A * A, Ab * Ab);
    }
}

// ---- forward mode: tangents on the eight parameters and on lo and hi in, tangents of the four integrals out ----
struct IntJvpLds {
    JvpLds j;
    double brk[2][2][kTrajProblems];
    double T[kTrajProblems], d1_dot[kTrajProblems];
};

__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(4)))      // 123 VGPRs: without the hint 153
k_jvp_integrals(FromArrays stage, Spline8 dot, size_t n, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi,
                const double *__restrict__ lo_dot, const double *__restrict__ hi_dot, Out4 value_dot)
{
    __shared__ IntJvpLds L;
    auto stage_problem = [&](int q, size_t i) {
        const DirectedDurations d = stage_tangents(L.j, q, i, stage.s, dot);
        L.T[q] = d.t0 + d.t1;
        L.d1_dot[q] = d.t1d;
        stage_breaks(L.brk, q, L.j.c, 1, 2, 3, d.t0, d.t1);
    };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        // one query, one segment at a time (loops the compiler is told to keep: the two queries of a pair and their two segments, taken at
        // once, cost more than the 128 registers of four waves per SIMD)
        auto query = [&](int q, double lo_q, double hi_q, double lo_d, double hi_d, double out[4]) {
            const double d0 = L.j.d0[q], d0d = L.j.d0_dot[q], d1d = L.d1_dot[q];
            const Window win = clamp_window(lo_q, hi_q, L.T[q]);
            const double a_dot = win.lo_taken ? lo_d : 0.0;
            double sum[4] = {0.0, 0.0, 0.0, 0.0};
#pragma nounroll
            for (int seg = 0; seg < 2; ++seg) {
                const SegmentConst c{L.j.c[seg][0][q], L.j.c[seg][1][q], L.j.c[seg][2][q], L.j.c[seg][3][q], L.brk[seg][0][q], L.brk[seg][1][q]};
                const Piece p = segment_piece(seg, win, d0);
                // the tangents of the piece's local ends, by where each end came from
                const double sad = seg ? (p.on && win.a > d0 ? a_dot - d0d : 0.0) : (p.on ? a_dot : 0.0);
                const double end0 = win.b > d0 ? d0d : (win.hi_taken ? hi_d : d0d + d1d), end1 = win.hi_taken ? hi_d - d0d : d1d;
                const double sbd = p.on ? (seg ? end1 : end0) : 0.0;
                const double x0d = L.j.t[seg][0][q], vad = L.j.t[seg][1][q], acc0d = L.j.t[seg][2][q], jrk0d = L.j.t[seg][3][q];
                segment_partials(c, p, [&](int i, double m0, double m1, double m2, double m3, double fa, double fb) {
                    // a partial that is 0 by structure is not a term
                    const double lead = i == 0 ? m0 * x0d + m1 * vad + m2 * acc0d : (i == 3 ? m2 * acc0d : m1 * vad + m2 * acc0d);
                    sum[i] += lead + m3 * jrk0d + fb * sbd - fa * sad;
                });
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) out[i] = win.ok ? sum[i] : quiet_nan();
        };
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double la, lb, ha, hb, lda = 0.0, ldb = 0.0, hda = 0.0, hdb = 0.0, a[4], b[4];
            load_window(lo, hi, e_first + e, two, la, lb, ha, hb);
            if (lo_dot) load_pair(lo_dot, e_first + e, two, lda, ldb);
            if (hi_dot) load_pair(hi_dot, e_first + e, two, hda, hdb);
#pragma nounroll
            for (int second = 0; second < 2; ++second) {
                double r[4];
                query(second ? qb : qa, second ? lb : la, second ? hb : ha, second ? ldb : lda, second ? hdb : hda, r);
#pragma unroll
                for (int i = 0; i < 4; ++i) { a[i] = second ? a[i] : r[i]; b[i] = r[i]; }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (value_dot.p[i]) store_pair(value_dot.p[i], e_first + e, a[i], b[i], two);
        });
    });
}

// ---- reverse mode: reduce_rows over ten sums: the four per segment that segment_chain takes, and what the window's ends put on duration0
// and on duration1.  A query whose output is NaN counts with upstream gradients of zero.
struct IntVjpLds {
    VjpLds v;
    double x0[2][kTrajProblems];
    double brk[2][2][kTrajProblems];
    double T[kTrajProblems];
};

__global__ void __launch_bounds__(kTrajBlock)
k_vjp_integrals(FromArrays stage, size_t n, size_t k, int P, int G, const double *__restrict__ lo, const double *__restrict__ hi, In4 g,
                SplineBar8 bar, double *__restrict__ lo_bar, double *__restrict__ hi_bar)
{
    __shared__ IntVjpLds L;
    auto stage_problem = [&](int q, size_t i) {
        Knots kn = stage.load(i);
        kn.check();
        stage_vjp(L.v, q, kn);
        L.x0[0][q] = kn.p0;
        L.x0[1][q] = kn.p1;
        L.T[q] = kn.t0 + kn.t1;
        stage_breaks(L.brk, q, L.v.c, 0, 3, 4, kn.t0, kn.t1);
    };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        // one query, one segment at a time (a loop the compiler is told to keep, as the pair's below: registers).  S: the ten sums
        auto query = [&](int q, double lo_q, double hi_q, double g0, double g1, double g2, double g3, double *S, double &lo_b, double &hi_b) {
            const double d0 = L.v.d0[q];
            const Window win = clamp_window(lo_q, hi_q, L.T[q]);
            const double g[4] = {win.ok ? g0 : 0.0, win.ok ? g1 : 0.0, win.ok ? g2 : 0.0, win.ok ? g3 : 0.0};
            double Ea0 = 0.0, Ea1 = 0.0, Eb0 = 0.0, Eb1 = 0.0;
            bool on0 = false, on1 = false;
#pragma nounroll
            for (int seg = 0; seg < 2; ++seg) {
                const SegmentConst c{L.x0[seg][q], L.v.c[seg][0][q], L.v.c[seg][3][q], L.v.c[seg][4][q], L.brk[seg][0][q], L.brk[seg][1][q]};
                const Piece p = segment_piece(seg, win, d0);
                double W[4] = {0.0, 0.0, 0.0, 0.0}, ea = 0.0, eb = 0.0;
                segment_partials(c, p, [&](int i, double m0, double m1, double m2, double m3, double fa, double fb) {
                    // a partial that is 0 by structure is not a term; the first term of a sum starts it
                    if (i == 0) { W[0] = g[0] * m0; W[1] = g[0] * m1; W[2] = g[0] * m2; W[3] = g[0] * m3; ea = g[0] * fa; eb = g[0] * fb; return; }
                    if (i < 3) W[1] += g[i] * m1;
                    W[2] += g[i] * m2;
                    W[3] += g[i] * m3;
                    ea += g[i] * fa;
                    eb += g[i] * fb;
                });
#pragma unroll
                for (int f = 0; f < 4; ++f) { S[f] += seg ? 0.0 : W[f]; S[4 + f] += seg ? W[f] : 0.0; }
                Ea0 = seg ? Ea0 : ea; Ea1 = seg ? ea : Ea1;
                Eb0 = seg ? Eb0 : eb; Eb1 = seg ? eb : Eb1;
                on0 = seg ? on0 : p.on; on1 = seg ? p.on : on1;
            }
            const bool knot = on0 && win.b > d0, end0_b = on0 && !knot;      // segment 0 ends on the knot | at b
            const double a1 = on1 && win.a > d0 && win.lo_taken ? Ea1 : 0.0;
            S[8] += ((knot || (end0_b && !win.hi_taken) ? Eb0 : 0.0) + a1) - (on1 && win.hi_taken ? Eb1 : 0.0);
            S[9] += (on1 && !win.hi_taken ? Eb1 : 0.0) + (end0_b && !win.hi_taken ? Eb0 : 0.0);
            lo_b = -((on0 && win.lo_taken ? Ea0 : 0.0) + a1);
            hi_b = (end0_b && win.hi_taken ? Eb0 : 0.0) + (on1 && win.hi_taken ? Eb1 : 0.0);
        };
        reduce_rows<10>(G, here, p_first, k, [&](int q, size_t at, bool two, double *S) {
            double la, lb, ha, hb, ga[4] = {0.0, 0.0, 0.0, 0.0}, gb[4] = {0.0, 0.0, 0.0, 0.0}, ba, bb, ca, cb;
            load_window(lo, hi, at, two, la, lb, ha, hb);
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (g.p[i]) load_pair(g.p[i], at, two, ga[i], gb[i]);
#pragma nounroll
            for (int second = 0; second < (two ? 2 : 1); ++second) {
                double b, c;
                query(q, second ? lb : la, second ? hb : ha, second ? gb[0] : ga[0], second ? gb[1] : ga[1], second ? gb[2] : ga[2],
                      second ? gb[3] : ga[3], S, b, c);
                ba = second ? ba : b; bb = b;
                ca = second ? ca : c; cb = c;
            }
            if (lo_bar) store_pair(lo_bar, at, ba, bb, two);
            if (hi_bar) store_pair(hi_bar, at, ca, cb, two);
        }, [&](int q, const double *S) {
            const SegmentBar a = segment_chain(L.v, 0, q, S[0], S[1], S[2], S[3]);
            const SegmentBar b = segment_chain(L.v, 1, q, S[4], S[5], S[6], S[7]);
            route_bars(L.v.bar, q, a, b, a.h + S[8], b.h + S[9]);
        });
        write_bars(L.v.bar, bar, p_first, here);
    });
}

// ---- second order: the derivative of the integrals' reverse rule along a direction (rp_trajectory_integrals_hvp) ----
// The upstream gradients g are held fixed; the direction is (x0d, vad, acc0d, jrk0d) on a segment's constants (stage_directed) and (sad, sbd)
// on the piece's local ends, by where each end came from, as in k_jvp_integrals; everything that routes -- lo_taken, hi_taken, which segment
// contributes, where segment 0 ends -- is the forward's.  For one segment's contribution I(C; sa, sb) with integrand f and phi = d vel / d C
// = (0, 1, s, s^2 / 2), with pos_d, vel_d, acc_d the direction's own cubic at a fixed local time and Nm the integral of s^m over the piece:
//     (dI / dC)_dot = (d2I / dC2) C_dot + (df(sb) / dC) sbd - (df(sa) / dC) sad
//     f(end)_dot    = (df(end) / dC) C_dot + f'(end) end_dot                  f' = vel, sign(vel) acc, 2 vel acc, 2 acc jrk0
//     d2I / dC2     = 0 (pos_int), 2 the integral of phi_i phi_j (vel_sq: N0 .. N4), the same with d acc / d C = (0, 0, 1, s) (acc_sq: N0 .. N2)
//     distance      piece by piece 0, but the sign of vel turns at its roots: a breakpoint c of velocity_breaks that is a root (c1 != 0,
//                   c2 != h) strictly inside the piece (sa < c < sa + w) adds 2 vel_d(c) / |acc(c)| (1, c, c^2 / 2) to the three dotted
//                   partials; acc(c) == 0 (a touch) adds nothing.  The factor 2 vel_d(c) / |acc(c)| is the problem's: staged, no division
//                   per query.  sign(vel) at an end of the piece is the segment's first sign turned once per root passed (staged too),
//                   not the sign of the end's own velocity, which at a rest end is rounding
// segment_partials_dot hands these out one output at a time; segment_partials gives the first-order partials in (acc0, jrk0) beside them.
// reduce_rows over fourteen sums.  Per segment S_a and S_j (the reverse rule's own: segment_chain's coefficients depend on h, and their
// derivative multiplies them; S_x and S_v enter it with constant coefficients and are in no derivative) and the dotted S_xd, S_vd, S_ad,
// S_jd -- S_xd because here the sum of g dpos_int / dx0 = g w has a derivative, g (sbd - sad), which the evaluator's rule has not: it goes
// to x0_bar_dot next to segment_chain_dot's; and the two dotted end terms for duration0 and duration1.
struct WinHvpLds {
    HvpLds h;
    double x0[2][kTrajProblems], x0d[2][kTrajProblems];
    double brk[2][2][kTrajProblems];      // per segment: c1, c2
    double root[2][2][kTrajProblems];     // the breakpoints that are roots of the velocity (c1 != 0, c2 != h); NaN: none
    double rt[2][2][kTrajProblems];       // 2 vel_d(c) / |acc(c)| there; 0 where there is no root, acc(c) == 0 or the quotient is not finite
    double s0[2][kTrajProblems];          // the sign of the velocity from the segment's start to its first root
    double T[kTrajProblems], d1_dot[kTrajProblems];
};

// the direction on one segment's constants and on the piece's local ends, and the staged root factors
struct SegmentDot { double x0d, vad, acc0d, jrk0d, sad, sbd, root1, root2, r1, r2, s0; };

// The dotted partials of one segment's contributions: each(i, n0, n1, n2, n3, fad, fbd) gets output i's (dI / dC)_dot in (x0, va, acc0,
// jrk0) and its integrand's derivative along the direction at the piece's start and end, one output at a time in the outputs' order.
// Without DIST the roots are not looked at.
template <bool DIST, class Each>
__device__ __forceinline__ void segment_partials_dot(const SegmentConst &c, const Piece &p, const SegmentDot &d, Each each)
{
    const double w = p.w, sa = p.sa, sb = sa + w, J = c.jrk0, third = 1.0 / 3.0;
    double X, V, A;
    local_state(c, sa, X, V, A);
    const double Vb = V + w * (A + (w * 0.5) * J), Ab = A + w * J;
    // the direction's cubic at the two ends, and the tangents of vel and acc there
    const double vda = cubic_vel(d.vad, d.acc0d, d.jrk0d, sa), vdb = cubic_vel(d.vad, d.acc0d, d.jrk0d, sb);
    const double ada = cubic_acc(d.acc0d, d.jrk0d, sa), adb = cubic_acc(d.acc0d, d.jrk0d, sb);
    const double Va_dot = vda + A * d.sad, Vb_dot = vdb + Ab * d.sbd;
    const double ha = sa * (sa * 0.5), hb = sb * (sb * 0.5);      // s^2 / 2 at the ends
    {
        const double ta = ha * (sa * third), tb = hb * (sb * third);
        each(0, d.sbd - d.sad, sb * d.sbd - sa * d.sad, hb * d.sbd - ha * d.sad, tb * d.sbd - ta * d.sad,
             cubic_pos(d.x0d, d.vad, d.acc0d, d.jrk0d, sa) + V * d.sad, cubic_pos(d.x0d, d.vad, d.acc0d, d.jrk0d, sb) + Vb * d.sbd);
    }
    {
        // the sign of the velocity just inside each end: the segment's first sign, turned once per root passed (a root on the start is
        // passed, one on the end is not: the same count that decides below which roots lie inside).  Not the sign of V or Vb themselves:
        // at a rest end they are of rounding size, and |vel| there is the continuation from inside
        const bool odd_a = (d.root1 <= sa) != (d.root2 <= sa), odd_b = (d.root1 < sb) != (d.root2 < sb);
        const double ga = odd_a ? -d.s0 : d.s0, gb = odd_b ? -d.s0 : d.s0;
        const double ea = ga * d.sad, eb = gb * d.sbd;
        double n1 = eb - ea, n2 = sb * eb - sa * ea, n3 = hb * eb - ha * ea;
        if (DIST) {
            const double r1 = d.root1 > sa && d.root1 < sb ? d.r1 : 0.0, r2 = d.root2 > sa && d.root2 < sb ? d.r2 : 0.0;
            n1 += r1 + r2;
            n2 += c.c1 * r1 + c.c2 * r2;
            n3 += (c.c1 * (c.c1 * 0.5)) * r1 + (c.c2 * (c.c2 * 0.5)) * r2;
        }
        each(1, 0.0, n1, n2, n3, ga * Va_dot, gb * Vb_dot);
    }
    const double N1 = w * (sa + w * 0.5), N2 = w * (sa * sa + w * (sa + w * third));
    {
        const double s2 = sa * sa;
        const double N3 = w * (s2 * sa + w * (1.5 * s2 + w * (sa + w * 0.25)));
        const double N4 = w * (s2 * s2 + w * (2.0 * (s2 * sa) + w * (2.0 * s2 + w * (sa + w * 0.2))));
        const double hj = 0.5 * d.jrk0d, ea = (2.0 * V) * d.sad, eb = (2.0 * Vb) * d.sbd;
        each(2, 0.0, 2.0 * (w * d.vad + N1 * d.acc0d + N2 * hj) + (eb - ea), 2.0 * (N1 * d.vad + N2 * d.acc0d + N3 * hj) + (sb * eb - sa * ea),
             (N2 * d.vad + N3 * d.acc0d + N4 * hj) + (hb * eb - ha * ea), (2.0 * V) * Va_dot, (2.0 * Vb) * Vb_dot);
    }
    {
        const double ea = (2.0 * A) * d.sad, eb = (2.0 * Ab) * d.sbd;
        each(3, 0.0, 0.0, 2.0 * (w * d.acc0d + N1 * d.jrk0d) + (eb - ea), 2.0 * (N1 * d.acc0d + N2 * d.jrk0d) + (sb * eb - sa * ea),
             (2.0 * A) * (ada + J * d.sad), (2.0 * Ab) * (adb + J * d.sbd));
    }
}

// S: the fourteen sums -- segment 0's S_a, S_j, S_xd, S_vd, S_ad, S_jd, segment 1's, then duration0's and duration1's dotted end terms
template <bool DIST>
__device__ __forceinline__ void window_hvp_query(const WinHvpLds &L, int q, double lo_q, double hi_q, double lo_d, double hi_d, const double (&g_in)[4],
                                                 double *S, double &lo_b, double &hi_b)
{
    const double d0 = L.h.d0[q], d0d = L.h.d0_dot[q], d1d = L.d1_dot[q];
    const Window win = clamp_window(lo_q, hi_q, L.T[q]);
    const double a_dot = win.lo_taken ? lo_d : 0.0;
    const double g[4] = {win.ok ? g_in[0] : 0.0, win.ok ? g_in[1] : 0.0, win.ok ? g_in[2] : 0.0, win.ok ? g_in[3] : 0.0};
    double Ea0 = 0.0, Ea1 = 0.0, Eb0 = 0.0, Eb1 = 0.0;
    bool on0 = false, on1 = false;
#pragma nounroll
    for (int seg = 0; seg < 2; ++seg) {
        const SegmentConst c{L.x0[seg][q], L.h.c[seg][0][q], L.h.c[seg][3][q], L.h.c[seg][4][q], L.brk[seg][0][q], L.brk[seg][1][q]};
        const Piece p = segment_piece(seg, win, d0);
        // the tangents of the piece's local ends, by where each end came from (k_jvp_integrals')
        const double sad = seg ? (p.on && win.a > d0 ? a_dot - d0d : 0.0) : (p.on ? a_dot : 0.0);
        const double end0 = win.b > d0 ? d0d : (win.hi_taken ? hi_d : d0d + d1d), end1 = win.hi_taken ? hi_d - d0d : d1d;
        const double sbd = p.on ? (seg ? end1 : end0) : 0.0;
        const SegmentDot d{L.x0d[seg][q], L.h.t[seg][0][q], L.h.t[seg][3][q], L.h.t[seg][4][q], sad, sbd, L.root[seg][0][q], L.root[seg][1][q],
                           L.rt[seg][0][q], L.rt[seg][1][q], L.s0[seg][q]};
        double W2 = 0.0, W3 = 0.0;
        segment_partials<DIST>(c, p, [&](int i, double, double, double m2, double m3, double, double) {
            if (i == 0) { W2 = g[0] * m2; W3 = g[0] * m3; return; }
            W2 += g[i] * m2;
            W3 += g[i] * m3;
        });
        double D[4] = {0.0, 0.0, 0.0, 0.0}, ea = 0.0, eb = 0.0;
        segment_partials_dot<DIST>(c, p, d, [&](int i, double n0, double n1, double n2, double n3, double fad, double fbd) {
            // a partial that is 0 by structure is not a term; the first term of a sum starts it
            if (i == 0) { D[0] = g[0] * n0; D[1] = g[0] * n1; D[2] = g[0] * n2; D[3] = g[0] * n3; ea = g[0] * fad; eb = g[0] * fbd; return; }
            if (i < 3) D[1] += g[i] * n1;
            D[2] += g[i] * n2;
            D[3] += g[i] * n3;
            ea += g[i] * fad;
            eb += g[i] * fbd;
        });
        S[0] += seg ? 0.0 : W2; S[1] += seg ? 0.0 : W3;
        S[6] += seg ? W2 : 0.0; S[7] += seg ? W3 : 0.0;
#pragma unroll
        for (int f = 0; f < 4; ++f) { S[2 + f] += seg ? 0.0 : D[f]; S[8 + f] += seg ? D[f] : 0.0; }
        Ea0 = seg ? Ea0 : ea; Ea1 = seg ? ea : Ea1;
        Eb0 = seg ? Eb0 : eb; Eb1 = seg ? eb : Eb1;
        on0 = seg ? on0 : p.on; on1 = seg ? p.on : on1;
    }
    // k_vjp_integrals' routing of the end terms, dotted
    const bool knot = on0 && win.b > d0, end0_b = on0 && !knot;
    const double a1 = on1 && win.a > d0 && win.lo_taken ? Ea1 : 0.0;
    S[12] += ((knot || (end0_b && !win.hi_taken) ? Eb0 : 0.0) + a1) - (on1 && win.hi_taken ? Eb1 : 0.0);
    S[13] += (on1 && !win.hi_taken ? Eb1 : 0.0) + (end0_b && !win.hi_taken ? Eb0 : 0.0);
    lo_b = -((on0 && win.lo_taken ? Ea0 : 0.0) + a1);
    hi_b = (end0_b && win.hi_taken ? Eb0 : 0.0) + (on1 && win.hi_taken ? Eb1 : 0.0);
}

template <bool DIST>
__device__ __forceinline__ void window_hvp_rows(WinHvpLds &L, int G, int here, size_t p_first, size_t k, const double *__restrict__ lo,
                                                const double *__restrict__ hi, const In4 &g, const double *__restrict__ lo_dot,
                                                const double *__restrict__ hi_dot, double *__restrict__ lo_bar_dot, double *__restrict__ hi_bar_dot)
{
    reduce_rows<14>(G, here, p_first, k, [&](int q, size_t at, bool two, double *S) {
        double la, lb, ha, hb, lda = 0.0, ldb = 0.0, hda = 0.0, hdb = 0.0, ga[4] = {0.0, 0.0, 0.0, 0.0}, gb[4] = {0.0, 0.0, 0.0, 0.0}, ba, bb, ca, cb;
        load_window(lo, hi, at, two, la, lb, ha, hb);
        if (lo_dot) load_pair(lo_dot, at, two, lda, ldb);
        if (hi_dot) load_pair(hi_dot, at, two, hda, hdb);
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (g.p[i]) load_pair(g.p[i], at, two, ga[i], gb[i]);
#pragma nounroll
        for (int second = 0; second < (two ? 2 : 1); ++second) {
            double b, c;
            const double gq[4] = {second ? gb[0] : ga[0], second ? gb[1] : ga[1], second ? gb[2] : ga[2], second ? gb[3] : ga[3]};
            window_hvp_query<DIST>(L, q, second ? lb : la, second ? hb : ha, second ? ldb : lda, second ? hdb : hda, gq, S, b, c);
            ba = second ? ba : b; bb = b;
            ca = second ? ca : c; cb = c;
        }
        if (lo_bar_dot) store_pair(lo_bar_dot, at, ba, bb, two);
        if (hi_bar_dot) store_pair(hi_bar_dot, at, ca, cb, two);
    }, [&](int q, const double *S) {
        SegmentBar a = segment_chain_dot(L.h, 0, q, S, S + 3);
        SegmentBar b = segment_chain_dot(L.h, 1, q, S + 6, S + 9);
        a.x0 += S[2];
        b.x0 += S[8];
        route_bars(L.h.bar, q, a, b, a.h + S[12], b.h + S[13]);
    });
}

__global__ void __launch_bounds__(kTrajBlock)
k_window_hvp(FromArrays stage, Spline8 dot, size_t n, size_t k, int P, int G, const double *__restrict__ lo, const double *__restrict__ hi, In4 g,
             const double *__restrict__ lo_dot, const double *__restrict__ hi_dot, SplineBar8 bar, double *__restrict__ lo_bar_dot,
             double *__restrict__ hi_bar_dot)
{
    __shared__ WinHvpLds L;
    const bool dist = g.p[1] != nullptr;      // uniform
    auto stage_problem = [&](int q, size_t i) {
        const DirectedDurations d = stage_hvp(L.h, q, i, stage.s, dot);
        L.T[q] = d.t0 + d.t1;
        L.d1_dot[q] = d.t1d;
#pragma unroll
        for (int seg = 0; seg < 2; ++seg) {
            const double *px0d = seg ? dot.p[1] : dot.p[0];
            L.x0[seg][q] = (seg ? stage.s.p[1] : stage.s.p[0])[i];
            L.x0d[seg][q] = px0d ? px0d[i] : 0.0;
        }
        stage_breaks(L.brk, q, L.h.c, 0, 3, 4, d.t0, d.t1, [&](int seg, double h, double c1, double c2) {
            const double va = L.h.c[seg][0][q], acc0 = L.h.c[seg][3][q], jrk0 = L.h.c[seg][4][q];
            const double vad = L.h.t[seg][0][q], acc0d = L.h.t[seg][3][q], jrk0d = L.h.t[seg][4][q];
            const bool root1 = c1 != 0.0, root2 = c2 != h;
            auto factor = [&](double c, bool root) {
                const double acc = cubic_acc(acc0, jrk0, c);
                const double f = root && acc != 0.0 ? 2.0 * cubic_vel(vad, acc0d, jrk0d, c) / abs_(acc) : 0.0;
                return finite_(f) ? f : 0.0;
            };
            L.root[seg][0][q] = root1 ? c1 : quiet_nan();
            L.root[seg][1][q] = root2 ? c2 : quiet_nan();
            L.rt[seg][0][q] = factor(c1, root1);
            L.rt[seg][1][q] = factor(c2, root2);
            // the first sign: that of the velocity at the middle of the longest of the three pieces (far from every root), turned back by
            // the roots before it
            const double l0 = c1, l1 = c2 - c1, l2 = h - c2;
            const int piece = l0 >= l1 && l0 >= l2 ? 0 : (l1 >= l2 ? 1 : 2);
            const double mid = piece == 0 ? 0.5 * c1 : (piece == 1 ? c1 + 0.5 * l1 : c2 + 0.5 * l2);
            const double v = cubic_vel(va, acc0, jrk0, mid), sign = v > 0.0 ? 1.0 : (v < 0.0 ? -1.0 : 0.0);
            const bool turned = (piece >= 1 && root1) != (piece == 2 && root2);
            L.s0[seg][q] = turned ? -sign : sign;
        });
    };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        // the walk over the monotone pieces and the roots: not taken where the distance has no gradient
        if (dist) window_hvp_rows<true>(L, G, here, p_first, k, lo, hi, g, lo_dot, hi_dot, lo_bar_dot, hi_bar_dot);
        else window_hvp_rows<false>(L, G, here, p_first, k, lo, hi, g, lo_dot, hi_dot, lo_bar_dot, hi_bar_dot);
        write_bars(L.h.bar, bar, p_first, here);
    });
}

// ---- how close two splines get: the extreme gap over a window (rp_trajectory_gap) ----
// D(t) = pos_A(t) - pos_B(t - delay) on the common domain [S, E], S = delay > 0 ? delay : +0.0, E = min(T_A, delay + T_B): a piecewise
// cubic whose pieces end at A's knot k_A = duration0_A and at B's, k_B = delay + duration0_B.  A query clamps its window to [a, b] inside
// [S, E], clamps the two knots (in time order, k_A first among equals) into [a, b] -- a knot outside leaves a piece of length zero, which
// has no root strictly inside -- and walks a, then per piece the roots of the relative velocity and the knot that ends it (if it lies in
// [a, b]), then b.  On a piece with left end c the relative velocity is a quadratic in u = t - c whose constants are the difference of the
// two selected segments' (vel, acc, jrk0) at c (A's segment 1 if k_A <= c, local time c - k_A; B's if k_B <= c, local time c - k_B, else
// c - delay); its roots are velocity_roots', candidates where strictly inside (0, the piece's length) and, as times c + u, strictly
// inside (a, b); the smaller first.  Every candidate's value is eval_query of A at its time minus eval_query of B at time - delay, the walk
// is the extrema's (Extreme::take: strict, the earliest among equals, a NaN never) and the time that comes back carries its candidate's
// own bits.  Selects only; the three pieces are a loop of three trips that the compiler is told to keep (registers: eleven candidates of
// two evaluations each per query, two queries per thread).  The block's first P threads leave per problem the two splines' evaluator
// constants, T_A and T_B.
struct GapLds {
    EvalLds a, b;
    double Ta[kTrajProblems], Tb[kTrajProblems];
};

__device__ __forceinline__ double gap_at(const GapLds &L, int q, double t, double delay)
{
    double pa, pb, vel, acc;
    eval_query(L.a, q, t, pa, vel, acc);
    eval_query(L.b, q, t - delay, pb, vel, acc);
    return pa - pb;
}

// one spline's (vel, acc, jrk0) in segment seg at local time s
__device__ __forceinline__ void local_motion(const EvalLds &L, int seg, int q, double s, double &vel, double &acc, double &jrk0)
{
    const double va = L.c[seg][1][q], acc0 = L.c[seg][2][q];
    jrk0 = L.c[seg][3][q];
    vel = cubic_vel(va, acc0, jrk0, s);
    acc = cubic_acc(acc0, jrk0, s);
}

__device__ __forceinline__ void gap_query(const GapLds &L, int q, double lo, double hi, double delay, Extreme &X)
{
    const double nan = quiet_nan();
    X = Extreme{nan, nan, nan, nan};
    const double kA = L.a.d0[q], kB = delay + L.b.d0[q], TA = L.Ta[q], EB = delay + L.Tb[q];
    const double S = delay > 0.0 ? delay : 0.0, E = EB < TA ? EB : TA;      // the common domain; T_A among equals
    const double a = lo > S ? lo : (lo != lo ? lo : S), b = hi < E ? hi : (hi != hi ? hi : E);      // clamp_window's rule from S on
    const bool ok = a <= b && finite_(delay) && EB == EB;      // a NaN or infinite delay, spline B under the NaN rule: nothing
    const bool b_first = kB < kA;      // the knots in time order, k_A first among equals
    X.take(ok, a, gap_at(L, q, a, delay));
    double c = a;
#pragma nounroll
    for (int piece = 0; piece < 3; ++piece) {
        const double knot = (piece == 0) == b_first ? kB : kA;      // the knot that ends the piece (the last piece ends at b)
        const bool inside = piece < 2 && ok && a <= knot && knot <= b;
        const double e = piece == 2 ? b : (knot < a ? a : (knot > b ? b : knot));
        const int seg_a = kA <= c, seg_b = kB <= c;
        double vel_a, acc_a, jrk_a, vel_b, acc_b, jrk_b, r0, r1;
        local_motion(L.a, seg_a, q, seg_a ? c - kA : c, vel_a, acc_a, jrk_a);
        local_motion(L.b, seg_b, q, seg_b ? c - kB : c - delay, vel_b, acc_b, jrk_b);
        velocity_roots(vel_a - vel_b, acc_a - acc_b, jrk_a - jrk_b, r0, r1);
        const double length = e - c, t0 = c + r0, t1 = c + r1;
        const bool in0 = ok && r0 > 0.0 && r0 < length && a < t0 && t0 < b, in1 = ok && r1 > 0.0 && r1 < length && a < t1 && t1 < b;
        const bool swap = in1 && (!in0 || r1 < r0);      // time order; a lone root comes first
        const double first = swap ? t1 : t0, second = swap ? t0 : t1;
        X.take(swap ? in1 : in0, first, gap_at(L, q, first, delay));
        X.take(swap ? in0 : in1, second, gap_at(L, q, second, delay));
        X.take(inside, knot, gap_at(L, q, knot, delay));
        c = e;
    }
    X.take(ok, b, gap_at(L, q, b, delay));
}

__global__ void __launch_bounds__(kTrajBlock)
k_gap(FromArrays a, FromArrays b, size_t n, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi,
      const double *__restrict__ delay, Out2 value, Out2 time)
{
    __shared__ GapLds L;
    auto stage_problem = [&](int q, size_t i) {
        Knots ka = a.load(i), kb = b.load(i);
        ka.check();
        kb.check();
        stage_eval(L.a, q, ka);
        stage_eval(L.b, q, kb);
        L.Ta[q] = ka.t0 + ka.t1;
        L.Tb[q] = kb.t0 + kb.t1;
    };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double la, lb, ha, hb, da = 0.0, db = 0.0;
            load_window(lo, hi, e_first + e, two, la, lb, ha, hb);
            if (delay) load_pair(delay, e_first + e, two, da, db);
            Extreme A, B;
            gap_query(L, qa, la, ha, da, A);
            gap_query(L, qb, lb, hb, db, B);
            if (value.p[0]) store_pair(value.p[0], e_first + e, A.lo_v, B.lo_v, two);
            if (value.p[1]) store_pair(value.p[1], e_first + e, A.hi_v, B.hi_v, two);
            if (time.p[0]) store_pair(time.p[0], e_first + e, A.lo_t, B.lo_t, two);
            if (time.p[1]) store_pair(time.p[1], e_first + e, A.hi_t, B.hi_t, two);
        });
    });
}

// ---- how far apart two splines are on average: the integrals of the gap D, of D^2 and of D'^2 over a window (rp_trajectory_tracking, _vjp,
// _jvp) ----
// D, the common domain, the clamped window [a, b], the two knots clamped into it and the segment each spline is in on a piece are k_gap's,
// in its expressions (track_window, track_pieces).  On a piece [c, e] with (X, V, A) the differences of the two selected segments' pos, vel,
// acc at their local starts s_A, s_B (the evaluator's expressions), J the difference of their jrk0 and w = e - c from the GLOBAL ends, each
// integral is a polynomial in w in shifted form from the piece's own start (track_values): no antiderivative is differenced.  A query's
// output is piece 0 + piece 1 + piece 2 in that order, exactly 0.0 where a == b, NaN where !(a <= b) or the NaN rule holds.  Selects only;
// the three pieces are a loop of three trips that the compiler is told to keep.
// The derivative rule.  For one piece, with C_A, C_B = (x0, va, acc0, jrk0) of the selected segments:
//     dI = S_i mA_i dC_A,i - S_i mB_i dC_B,i + P_A ds_A - P_B ds_B + f(w) dw
//     mA_i = the integral over u in [0, w] of g'(u) phi_i(s_A + u), mB_i the same with s_B
//     gap_int: g' = 1, phi = (1, s, s^2 / 2, s^3 / 6)      gap_sq: g' = 2 D, the same phi      relvel_sq: g' = 2 D', phi = (0, 1, s, s^2 / 2)
//     P_A = the integral of g' vel_A(s_A + u) (acc_A for relvel_sq), P_B likewise; f the integrand at the piece's end
// all polynomials in w from the local states at the piece's start (gap_moments, rate_moments); P_A - P_B = f(w) - f(0) holds, unused.  With
// s_A = c - off_A, s_B = c - off_B, w = e - c, off_A in {0, k_A}, off_B in {delay, k_B}, the tangent of a piece end is that of where it came
// from: a = lo -> lo, a = the clamp S = delay > 0 -> delay (START), a = +0.0 -> nothing; b = hi -> hi, b = T_A -> d0A + d1A (END_A, first among
// equals), b = delay + T_B -> delay + d0B + d1B (END_B); a knot k_A -> d0A, k_B -> delay + d0B; a knot clamped to an end carries that end's
// tangent (its piece has length zero; track_pieces names a piece end a, b, k_A or k_B, and the kernels resolve a and b once per query).
// f is continuous across a knot, so what an inner end carries cancels between its two pieces up to
// rounding: ties between classes change nothing.  START needs delay > 0: at a delay of exactly 0 the start is the constant +0.0 (the kink of
// section 18).  Forward mode contracts the rule with segment_tangents' tangents; reverse mode adds the m's, weighted by the upstream
// gradients, to segment_chain's four sums per segment and the end terms to two sums for the durations -- ten sums per spline, one spline per
// launch (k_tracking_vjp<SIDE>; side A's launch also writes lo_bar, hi_bar, delay_bar).
// Nine to thirteen n x k arrays travel through the two derivative kernels.  Left alone, the compiler carries one 64-bit address per array from
// element to element (and one per gradient row from trip to trip): some thirty registers that hold no data.  An element index that it cannot
// see through is added to each base where it is used instead: one instruction per access.
__device__ __forceinline__ size_t opaque_index(size_t at)
{
    asm volatile("" : "+v"(at));
    return at;
}

__device__ __forceinline__ int opaque_place(int q)
{
    asm volatile("" : "+v"(q));
    return q;
}

// (the same for what a thread derives from its own number once and would keep for the whole launch: a value of the trip instead)
__device__ __forceinline__ int opaque_uniform(int g)
{
    asm volatile("" : "+s"(g));
    return g;
}

using Out3 = Table<double, 3>;                 // gap_int, gap_sq, relvel_sq
using In3 = Table<const double, 3>;

struct TrackLds {
    EvalLds a, b;
    double Ta[kTrajProblems], Tb[kTrajProblems];
};

enum { kPtNone, kPtLo, kPtStart, kPtHi, kPtEndA, kPtEndB };      // where a window end came from
enum { kEndA, kEndB, kEndKnotA, kEndKnotB };                     // what a piece's end is: the window's a or b, or a knot inside it

struct TrackWindow {
    double a, b, kA, kB, delay;
    int cls_a, cls_b;
    bool ok, b_first;
};

// gap_query's domain, window and knots.  SAFE (the reverse rule): a query without an answer walks the empty window at 0 with a delay of 0,
// so that its terms are finite and count with upstream gradients of zero
template <bool SAFE>
__device__ __forceinline__ TrackWindow track_window(double d0A, double TA, double d0B, double TB, double lo, double hi, double delay)
{
    TrackWindow win;
    const double EB = delay + TB;
    const double S = delay > 0.0 ? delay : 0.0, E = EB < TA ? EB : TA;      // the common domain; T_A among equals
    win.a = lo > S ? lo : (lo != lo ? lo : S);
    win.b = hi < E ? hi : (hi != hi ? hi : E);
    win.ok = win.a <= win.b && finite_(delay) && EB == EB;
    win.cls_a = lo > S ? kPtLo : (delay > 0.0 ? kPtStart : kPtNone);
    win.cls_b = hi < E ? kPtHi : (EB < TA ? kPtEndB : kPtEndA);
    win.delay = delay;
    if (SAFE && !win.ok) win.a = win.b = win.delay = 0.0;
    win.kA = d0A;
    win.kB = win.delay + d0B;
    win.b_first = win.kB < win.kA;      // the knots in time order, k_A first among equals
    return win;
}

struct TrackPiece {
    double w, sA, sB;
    int seg_a, seg_b, cls_c, cls_e;
};

template <class Each> __device__ __forceinline__ void track_pieces(const TrackWindow &win, Each each)
{
    double c = win.a;
    int cls_c = kEndA;
#pragma nounroll
    for (int piece = 0; piece < 3; ++piece) {
        const bool kb = (piece == 0) == win.b_first;      // the knot that ends the piece (the last piece ends at b)
        const double knot = kb ? win.kB : win.kA;
        const bool before = knot < win.a, after = knot > win.b;
        const double e = piece == 2 ? win.b : (before ? win.a : (after ? win.b : knot));
        const int cls_e = piece == 2 ? kEndB : (before ? kEndA : (after ? kEndB : (kb ? kEndKnotB : kEndKnotA)));
        TrackPiece p;
        p.seg_a = win.kA <= c;
        p.seg_b = win.kB <= c;
        p.sA = p.seg_a ? c - win.kA : c;
        p.sB = p.seg_b ? c - win.kB : c - win.delay;
        p.w = e - c;
        p.cls_c = cls_c;
        p.cls_e = cls_e;
        each(p);
        c = e;
        cls_c = cls_e;
    }
}

// the two selected segments at their local starts: the gap's (X, V, A, J) and each side's own (vel, acc, jrk0)
struct TrackState { double X, V, A, J, VA, AA, JA, VB, AB, JB; };

__device__ __forceinline__ TrackState track_state(const SegmentConst &ca, const SegmentConst &cb, const TrackPiece &p)
{
    TrackState t;
    double XA, XB;
    local_state(ca, p.sA, XA, t.VA, t.AA);
    local_state(cb, p.sB, XB, t.VB, t.AB);
    t.JA = ca.jrk0;
    t.JB = cb.jrk0;
    t.X = XA - XB;
    t.V = t.VA - t.VB;
    t.A = t.AA - t.AB;
    t.J = t.JA - t.JB;
    return t;
}

__device__ __forceinline__ SegmentConst eval_const(const double (&c)[2][4][kTrajProblems], int seg, int q)
{
    return SegmentConst{c[seg][0][q], c[seg][1][q], c[seg][2][q], c[seg][3][q], 0.0, 0.0};
}

// one piece's contributions: the integrals over [0, w] of D, D^2, D'^2 with D(u) = X + V u + A u^2 / 2 + J u^3 / 6
__device__ __forceinline__ void track_values(const TrackState &t, double w, double v[3])
{
    const double X = t.X, V = t.V, A = t.A, J = t.J, third = 1.0 / 3.0;
    v[0] = w * (X + (w * 0.5) * (V + (w * third) * (A + (w * 0.25) * J)));
    const double t6 = (A * J) * (1.0 / 36.0) + w * ((J * J) * (1.0 / 252.0));
    const double t5 = ((A * A) * 0.25 + (V * J) * third) * 0.2 + w * t6;
    const double t4 = (V * A + (X * J) * third) * 0.25 + w * t5;
    const double t3 = (V * V + X * A) * third + w * t4;
    v[1] = w * (X * X + w * (X * V + w * t3));
    v[2] = w * (V * V + w * (V * A + (w * third) * ((A * A + V * J) + w * (0.75 * (A * J) + (0.15 * w) * (J * J)))));
}

__device__ __forceinline__ void tracking_query(const TrackLds &L, int q, double lo, double hi, double delay, double out[3])
{
    const TrackWindow win = track_window<false>(L.a.d0[q], L.Ta[q], L.b.d0[q], L.Tb[q], lo, hi, delay);
    double sum[3] = {0.0, 0.0, 0.0};
    track_pieces(win, [&](const TrackPiece &p) {
        double v[3];
        track_values(track_state(eval_const(L.a.c, p.seg_a, q), eval_const(L.b.c, p.seg_b, q), p), p.w, v);
#pragma unroll
        for (int i = 0; i < 3; ++i) sum[i] += v[i];
    });
#pragma unroll
    for (int i = 0; i < 3; ++i) out[i] = win.ok ? (win.a == win.b ? 0.0 : sum[i]) : quiet_nan();
}

__global__ void __launch_bounds__(kTrajBlock)
k_tracking(FromArrays a, FromArrays b, size_t n, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi,
           const double *__restrict__ delay, Out3 value)
{
    __shared__ TrackLds L;
    auto stage_problem = [&](int q, size_t i) {
        Knots ka = a.load(i), kb = b.load(i);
        ka.check();
        kb.check();
        stage_eval(L.a, q, ka);
        stage_eval(L.b, q, kb);
        L.Ta[q] = ka.t0 + ka.t1;
        L.Tb[q] = kb.t0 + kb.t1;
    };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double la, lb, ha, hb, da = 0.0, db = 0.0, A[3], B[3];
            load_window(lo, hi, e_first + e, two, la, lb, ha, hb);
            if (delay) load_pair(delay, e_first + e, two, da, db);
            tracking_query(L, qa, la, ha, da, A);
            tracking_query(L, qb, lb, hb, db, B);
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (value.p[i]) store_pair(value.p[i], e_first + e, A[i], B[i], two);
        });
    });
}

// The moments of one piece that both derivative rules are made of, one output at a time and in the outputs' order so that no more than one
// output's numbers are live: Em = the integral of D u^m, Qm = that of D' u^m over [0, w].  With phi_i(s + u) expanded in u the rule's sums
// regroup: S_i m_i dC_i = the integral of g'(u) times the tangent cubic of the segment at s + u, so with (Xd, Vd, Ad, Jd) the tangent of the
// piece's own (X, V, A, J) at fixed u -- the tangent cubics' local states at s_A, s_B, their difference, plus (vel, acc, jrk0) of each side
// times ds_A, ds_B --
//     d gap_int = Xd w + Vd w^2 / 2 + Ad w^3 / 6 + Jd w^4 / 24 + D(w) dw
//     d gap_sq = 2 (Xd E0 + Vd E1 + Ad E2 / 2 + Jd E3 / 6) + D(w)^2 dw            d relvel_sq = 2 (Vd Q0 + Ad Q1 + Jd Q2 / 2) + D'(w)^2 dw
// the same numbers as the rule's m_i and P, contracted in another order.  Reverse mode reads the same lines backwards: the upstream gradients
// weight the coefficients of (Xd, Vd, Ad, Jd) into (Xb, Vb, Ab, Jb), and a side's four sums are k_trajectory_vjp's w0 .. w3 of (Xb, Vb, Ab) at
// its local start, with Jb on the last.
__device__ __forceinline__ double piece_end_gap(const TrackState &t, double w) { return t.X + w * (t.V + (w * 0.5) * (t.A + (w * (1.0 / 3.0)) * t.J)); }
__device__ __forceinline__ double piece_end_rate(const TrackState &t, double w) { return t.V + w * (t.A + (w * 0.5) * t.J); }

__device__ __forceinline__ void gap_moments(const TrackState &t, double w, double &E0, double &E1, double &E2, double &E3)
{
    const double X = t.X, V = t.V, A = t.A, J = t.J, w2 = w * w;
    E0 = w * (X + w * (V * 0.5 + w * (A * (1.0 / 6.0) + (w * (1.0 / 24.0)) * J)));
    E1 = w2 * (X * 0.5 + w * (V * (1.0 / 3.0) + w * (A * 0.125 + (w * (1.0 / 30.0)) * J)));
    E2 = (w2 * w) * (X * (1.0 / 3.0) + w * (V * 0.25 + w * (A * 0.1 + (w * (1.0 / 36.0)) * J)));
    E3 = (w2 * w2) * (X * 0.25 + w * (V * 0.2 + w * (A * (1.0 / 12.0) + (w * (1.0 / 42.0)) * J)));
}

__device__ __forceinline__ void rate_moments(const TrackState &t, double w, double &Q0, double &Q1, double &Q2)
{
    const double V = t.V, A = t.A, J = t.J;
    Q0 = w * (V + (w * 0.5) * (A + (w * (1.0 / 3.0)) * J));
    Q1 = (w * w) * (V * 0.5 + w * (A * (1.0 / 3.0) + (w * 0.125) * J));
    Q2 = (w * w * w) * (V * (1.0 / 3.0) + w * (A * 0.25 + (w * 0.1) * J));
}

// ---- forward mode: tangents on both splines' eight parameters and on lo, hi, delay in, tangents of the three integrals out ----
struct TrackJvpLds {
    JvpLds a, b;
    double Ta[kTrajProblems], Tb[kTrajProblems], Ta_dot[kTrajProblems], Tb_dot[kTrajProblems];
};

__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(4)))
k_tracking_jvp(FromArrays a, FromArrays b, Spline8 a_dot, Spline8 b_dot, size_t n, size_t k, int P, const double *__restrict__ lo,
               const double *__restrict__ hi, const double *__restrict__ delay, const double *__restrict__ lo_dot,
               const double *__restrict__ hi_dot, const double *__restrict__ delay_dot, Out3 value_dot)
{
    __shared__ TrackJvpLds L;
    auto stage_problem = [&](int q, size_t at) {
        const size_t i = opaque_index(at);
        const DirectedDurations da = stage_tangents(L.a, q, i, a.s, a_dot);
        L.Ta[q] = da.t0 + da.t1;
        L.Ta_dot[q] = da.t0d + da.t1d;
        const DirectedDurations db = stage_tangents(L.b, q, i, b.s, b_dot);
        L.Tb[q] = db.t0 + db.t1;
        L.Tb_dot[q] = db.t0d + db.t1d;
    };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        auto query = [&](int q, double lo_q, double hi_q, double dl_q, double lo_d, double hi_d, double dl_d, double out[3]) {
            const TrackWindow win = track_window<false>(L.a.d0[q], L.Ta[q], L.b.d0[q], L.Tb[q], lo_q, hi_q, dl_q);
            // the tangent of a piece end, by where it came from
            const double d0Ad = L.a.d0_dot[q], kBd = dl_d + L.b.d0_dot[q];
            const double ad = win.cls_a == kPtLo ? lo_d : (win.cls_a == kPtStart ? dl_d : 0.0);
            const double bd = win.cls_b == kPtHi ? hi_d : (win.cls_b == kPtEndA ? L.Ta_dot[q] : dl_d + L.Tb_dot[q]);
            auto tangent = [&](int cls) { return cls == kEndA ? ad : (cls == kEndB ? bd : (cls == kEndKnotA ? d0Ad : kBd)); };
            double sum[3] = {0.0, 0.0, 0.0};
            track_pieces(win, [&](const TrackPiece &p) {
                const TrackState t = track_state(eval_const(L.a.c, p.seg_a, q), eval_const(L.b.c, p.seg_b, q), p);
                const double cd = tangent(p.cls_c), ed = tangent(p.cls_e);
                const double dsA = cd - (p.seg_a ? d0Ad : 0.0), dsB = cd - (p.seg_b ? kBd : dl_d), dw = ed - cd;
                // the tangent cubics' local states, and the tangent of the piece's own state at fixed u
                double XAd, VAd, AAd, XBd, VBd, ABd;
                const SegmentConst da = eval_const(L.a.t, p.seg_a, q), db = eval_const(L.b.t, p.seg_b, q);
                local_state(da, p.sA, XAd, VAd, AAd);
                local_state(db, p.sB, XBd, VBd, ABd);
                const double Xd = (XAd - XBd) + (t.VA * dsA - t.VB * dsB), Vd = (VAd - VBd) + (t.AA * dsA - t.AB * dsB);
                const double Ad = (AAd - ABd) + (t.JA * dsA - t.JB * dsB), Jd = da.jrk0 - db.jrk0;
                const double w = p.w, Dw = piece_end_gap(t, w), Vw = piece_end_rate(t, w);
                sum[0] += w * (Xd + (w * 0.5) * (Vd + (w * (1.0 / 3.0)) * (Ad + (w * 0.25) * Jd))) + Dw * dw;
                {
                    double E0, E1, E2, E3;
                    gap_moments(t, w, E0, E1, E2, E3);
                    sum[1] += 2.0 * (Xd * E0 + Vd * E1 + (0.5 * Ad) * E2 + (Jd * (1.0 / 6.0)) * E3) + (Dw * Dw) * dw;
                }
                {
                    double Q0, Q1, Q2;
                    rate_moments(t, w, Q0, Q1, Q2);
                    sum[2] += 2.0 * (Vd * Q0 + Ad * Q1 + (0.5 * Jd) * Q2) + (Vw * Vw) * dw;
                }
            });
#pragma unroll
            for (int i = 0; i < 3; ++i) out[i] = win.ok ? sum[i] : quiet_nan();
        };
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            // (the pair's two queries one after the other, each with its own 8-byte loads -- the second's are cache hits: both queries' six
            // inputs held at once cost the registers that four waves per SIMD leave; the results leave as 16-byte pairs)
            const double inf = __builtin_inf();
            const size_t at = opaque_index(e_first + e);
            double A[3], B[3];
#pragma nounroll
            for (int second = 0; second < 2; ++second) {
                const size_t el = opaque_index(at + (two ? second : 0));
                double r[3];
                query(second ? qb : qa, lo ? lo[el] : -inf, hi ? hi[el] : inf, delay ? delay[el] : 0.0, lo_dot ? lo_dot[el] : 0.0,
                      hi_dot ? hi_dot[el] : 0.0, delay_dot ? delay_dot[el] : 0.0, r);
#pragma unroll
                for (int i = 0; i < 3; ++i) { A[i] = second ? A[i] : r[i]; B[i] = r[i]; }
            }
#pragma unroll
            for (int i = 0; i < 3; ++i)
                if (value_dot.p[i]) store_pair(value_dot.p[i], at, A[i], B[i], two);
        });
    });
}

// ---- reverse mode: one spline per launch (SIDE 0: A, 1: B).  reduce_rows over ten sums: the four per segment that segment_chain takes of
// the launch's own spline, and what the piece ends put on its duration0 and duration1.  Side A's launch writes lo_bar, hi_bar and delay_bar.
// A query whose outputs are NaN counts with upstream gradients of zero.
struct TrackVjpLds {
    VjpLds v;                           // the launch's own spline: segment_chain's constants and the eight results
    double x0[2][kTrajProblems];
    EvalLds o;                          // the other spline
    double Tv[kTrajProblems], To[kTrajProblems];
    double g[3][kTrajBlock];            // each thread's upstream gradients of the query it is at (read per piece, not kept in registers)
};

template <int SIDE>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(4)))
k_tracking_vjp(FromArrays a, FromArrays b, size_t n, size_t k, int P, int G, const double *__restrict__ lo, const double *__restrict__ hi,
               const double *__restrict__ delay, In3 g, SplineBar8 bar, double *__restrict__ lo_bar, double *__restrict__ hi_bar,
               double *__restrict__ delay_bar)
{
    __shared__ TrackVjpLds L;
    auto stage_problem = [&](int place, size_t at) {
        const int q = opaque_place(place);
        const size_t i = opaque_index(at);
        Knots own = SIDE ? b.load(i) : a.load(i), other = SIDE ? a.load(i) : b.load(i);
        own.check();
        other.check();
        stage_vjp(L.v, q, own);
        L.x0[0][q] = own.p0;
        L.x0[1][q] = own.p1;
        L.Tv[q] = own.t0 + own.t1;
        stage_eval(L.o, q, other);
        L.To[q] = other.t0 + other.t1;
    };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        // one query, one piece at a time.  S: the ten sums
        auto query = [&](int q, double lo_q, double hi_q, double dl_q, double g0, double g1, double g2, double *S, double &lo_b, double &hi_b,
                         double &dl_b) {
            const double d0v = L.v.d0[q], d0o = L.o.d0[q], Tv = L.Tv[q], To = L.To[q];
            const TrackWindow win = track_window<true>(SIDE ? d0o : d0v, SIDE ? To : Tv, SIDE ? d0v : d0o, SIDE ? Tv : To, lo_q, hi_q, dl_q);
            const int me = opaque_place((int)threadIdx.x);
            L.g[0][me] = win.ok ? g0 : 0.0;      // ok: of the query as given
            L.g[1][me] = win.ok ? g1 : 0.0;
            L.g[2][me] = win.ok ? g2 : 0.0;
            // what the window's a and b take, what the launch's own duration0 takes (its knot as a piece end and as an offset), what the delay
            // takes (B's knot and B's offset)
            double bar_a = 0.0, bar_b = 0.0, dl = 0.0, carry = 0.0;
            double &own0 = S[8];
            auto route = [&](int cls, double v) {
                bar_b += cls == kEndB ? v : 0.0;
                if (SIDE == 0) {
                    bar_a += cls == kEndA ? v : 0.0;
                    own0 += cls == kEndKnotA ? v : 0.0;
                    dl += cls == kEndKnotB ? v : 0.0;
                } else {
                    own0 += cls == kEndKnotB ? v : 0.0;
                }
            };
            track_pieces(win, [&](const TrackPiece &p) {
                const int seg_v = SIDE ? p.seg_b : p.seg_a, seg_o = SIDE ? p.seg_a : p.seg_b;
                auto state = [&](int at) {
                    const SegmentConst cv{L.x0[seg_v][at], L.v.c[seg_v][0][at], L.v.c[seg_v][3][at], L.v.c[seg_v][4][at], 0.0, 0.0};
                    const SegmentConst co = eval_const(L.o.c, seg_o, at);
                    return track_state(SIDE ? co : cv, SIDE ? cv : co, p);
                };
                // the gradients on the tangent of the piece's state, (Xb, Vb, Ab, Jb), and on its length, F
                const double gq[3] = {L.g[0][me], L.g[1][me], L.g[2][me]};
                const double w = p.w, w2 = w * (w * 0.5), w3 = w2 * (w * (1.0 / 3.0));
                double Xb = gq[0] * w, Vb = gq[0] * w2, Ab = gq[0] * w3, Jb = gq[0] * (w3 * (w * 0.25));
                {
                    const TrackState t = state(q);
                    {
                        double E0, E1, E2, E3;
                        gap_moments(t, w, E0, E1, E2, E3);
                        const double h = 2.0 * gq[1];
                        Xb += h * E0; Vb += h * E1; Ab += gq[1] * E2; Jb += gq[1] * (E3 * (1.0 / 3.0));
                    }
                    {
                        double Q0, Q1, Q2;
                        rate_moments(t, w, Q0, Q1, Q2);
                        const double h = 2.0 * gq[2];
                        Vb += h * Q0; Ab += h * Q1; Jb += gq[2] * Q2;
                    }
                }
                // the launch's own side: k_trajectory_vjp's weights at its local start; B enters the gap with a minus
                {
                    const double s = SIDE ? p.sB : p.sA, h2 = s * (s * 0.5), h3 = h2 * (s * (1.0 / 3.0));
                    const double W[4] = {Xb, Xb * s + Vb, Xb * h2 + Vb * s + Ab, Xb * h3 + Vb * h2 + Ab * s + Jb};
#pragma unroll
                    for (int f = 0; f < 4; ++f) {
                        const double Wf = SIDE ? -W[f] : W[f];
                        S[f] += seg_v ? 0.0 : Wf;
                        S[4 + f] += seg_v ? Wf : 0.0;
                    }
                }
                // the piece's state and each side's (vel, acc, jrk0) at its local start once more (read again, not kept: the moments above need
                // the registers)
                const TrackState t = state(opaque_place(q));
                const double Dw = piece_end_gap(t, w), Vw = piece_end_rate(t, w);
                const double F = gq[0] * Dw + gq[1] * (Dw * Dw) + gq[2] * (Vw * Vw);
                const double PA = Xb * t.VA + Vb * t.AA + Ab * t.JA, PB = Xb * t.VB + Vb * t.AB + Ab * t.JB;
                // ds_A = dc - doff_A, ds_B = dc - doff_B, dw = de - dc
                route(p.cls_c, carry + ((PA - PB) - F));
                carry = F;
                if (SIDE == 0) {
                    own0 -= p.seg_a ? PA : 0.0;
                    dl += PB;
                } else {
                    own0 += p.seg_b ? PB : 0.0;
                }
            });
            route(kEndB, carry);
            // ... and where each window end came from
            const bool own_end = win.cls_b == (SIDE ? kPtEndB : kPtEndA);
            S[8] += own_end ? bar_b : 0.0;
            S[9] += own_end ? bar_b : 0.0;
            if (SIDE == 0) {
                lo_b = win.cls_a == kPtLo ? bar_a : 0.0;
                hi_b = win.cls_b == kPtHi ? bar_b : 0.0;
                dl_b = (dl + (win.cls_a == kPtStart ? bar_a : 0.0)) + (win.cls_b == kPtEndB ? bar_b : 0.0);
            } else {
                lo_b = hi_b = dl_b = 0.0;
            }
        };
        // (a pair's two queries one after the other, each with its own 8-byte loads and stores: both queries' nine inputs and three results held
        // at once cost the registers of a wave per SIMD)
        reduce_rows<10>(opaque_uniform(G), here, p_first, k, [&](int q, size_t at, bool two, double *S) {
            const double inf = __builtin_inf();
#pragma nounroll
            for (int second = 0; second < (two ? 2 : 1); ++second) {
                const size_t el = opaque_index(at + second);
                double lo_b, hi_b, dl_b;
                query(q, lo ? lo[el] : -inf, hi ? hi[el] : inf, delay ? delay[el] : 0.0, g.p[0] ? g.p[0][el] : 0.0, g.p[1] ? g.p[1][el] : 0.0,
                      g.p[2] ? g.p[2][el] : 0.0, S, lo_b, hi_b, dl_b);
                if (SIDE == 0) {
                    if (lo_bar) lo_bar[el] = lo_b;
                    if (hi_bar) hi_bar[el] = hi_b;
                    if (delay_bar) delay_bar[el] = dl_b;
                }
            }
        }, [&](int q, const double *S) {
            const SegmentBar s0 = segment_chain(L.v, 0, q, S[0], S[1], S[2], S[3]);
            const SegmentBar s1 = segment_chain(L.v, 1, q, S[4], S[5], S[6], S[7]);
            route_bars(L.v.bar, q, s0, s1, s0.h + S[8], s1.h + S[9]);
        });
        // write_bars
        __syncthreads();
        if ((int)threadIdx.x < here) {
            const int me = opaque_place((int)threadIdx.x);
            const size_t i = p_first + (size_t)me;
#pragma unroll
            for (int f = 0; f < 8; ++f)
                if (bar.p[f]) bar.p[f][i] = L.v.bar[f][me];
        }
    });
}

// ---- second order: the derivative of the tracking integrals' reverse rule along a direction (rp_trajectory_tracking_hvp; DESIGN.md
// section 23) ----
// The upstream gradients g are held fixed; the direction is on both splines' eight parameters and on lo, hi, delay.  Everything that routes
// -- the classes of a and b, the order of the knots, which knot is clamped to which end, the segment each spline is in on a piece -- is the
// forward's, and every piece end is an affine function of lo, hi, delay and the durations with constant coefficients: the ends carry the
// forward rule's tangents (cd, ed) and have no second derivative.  Per piece the lines of k_tracking_vjp are differentiated one by one:
//     (Xd, Vd, Ad, Jd)   the tangent of the piece's state at fixed u (k_tracking_jvp's), wd = ed - cd
//     Em_dot = Em(Xd, Vd, Ad, Jd) + D(w) w^m wd        Qm_dot = Qm(Vd, Ad, Jd) + D'(w) w^m wd        (the moments are linear in the state)
//     (Xb, Vb, Ab, Jb)_dot from them, term by term; W[f]_dot = W[f] of the dotted four + W[f - 1] sd at the own local start s
//     P_A_dot, P_B_dot by the product rule with each side's own (vel, acc, jrk0)_dot = the tangent cubic's local state + (acc, jrk0, 0) ds
//     F_dot = (g0 + 2 g1 D(w)) (D_d(w) + D'(w) wd) + 2 g2 D'(w) (D'_d(w) + D''(w) wd)
// all polynomials in w from the piece's own start; nothing is divided per query.  reduce_rows over fourteen sums per side: S_a, S_j per
// segment (segment_chain's coefficients on them depend on h), the dotted S_xd, S_vd, S_ad, S_jd per segment (segment_chain_dot; S_xd goes
// to x0_bar_dot beside it) and the two dotted end terms of the durations.  One spline per launch as in k_tracking_vjp; side A's launch
// writes lo_bar_dot, hi_bar_dot and delay_bar_dot.  The upstream gradients stay in registers: the staged constants fill the LDS.
struct PairHvpLds {
    HvpLds h;                           // the launch's own spline: segment_chain_dot's constants, their tangents and the eight results
    double x0[2][kTrajProblems], x0d[2][kTrajProblems];
    JvpLds o;                           // the other spline's constants and tangents
    double Tv[kTrajProblems], To[kTrajProblems], Tvd[kTrajProblems], Tod[kTrajProblems];
};

template <int SIDE>
__global__ void __launch_bounds__(kTrajBlock)
k_pair_hvp(Spline8 a, Spline8 b, Spline8 a_dot, Spline8 b_dot, size_t n, size_t k, int P, int G, const double *__restrict__ lo,
           const double *__restrict__ hi, const double *__restrict__ delay, In3 g, const double *__restrict__ lo_dot,
           const double *__restrict__ hi_dot, const double *__restrict__ delay_dot, SplineBar8 bar, double *__restrict__ lo_bar_dot,
           double *__restrict__ hi_bar_dot, double *__restrict__ delay_bar_dot)
{
    __shared__ PairHvpLds L;
    auto stage_problem = [&](int place, size_t at) {
        const int q = opaque_place(place);
        const size_t i = opaque_index(at);
        const DirectedDurations dv = stage_directed(i, SIDE ? b : a, SIDE ? b_dot : a_dot, [&](int seg, const DirectedSegment &s) {
            L.h.c[seg][0][q] = s.va; L.h.c[seg][1][q] = s.vb; L.h.c[seg][2][q] = s.dx; L.h.c[seg][3][q] = s.acc0; L.h.c[seg][4][q] = s.jrk0;
            L.h.c[seg][5][q] = s.ih;
            L.h.t[seg][0][q] = s.vad; L.h.t[seg][1][q] = s.vbd; L.h.t[seg][2][q] = s.dxd; L.h.t[seg][3][q] = s.acc0d; L.h.t[seg][4][q] = s.jrk0d;
            L.h.t[seg][5][q] = s.hd;
            L.x0[seg][q] = s.x0;
            L.x0d[seg][q] = s.x0d;
        });
        L.h.d0[q] = dv.t0;
        L.h.d0_dot[q] = dv.t0d;
        L.Tv[q] = dv.t0 + dv.t1;
        L.Tvd[q] = dv.t0d + dv.t1d;
        const DirectedDurations dn = stage_tangents(L.o, q, i, SIDE ? a : b, SIDE ? a_dot : b_dot);
        L.To[q] = dn.t0 + dn.t1;
        L.Tod[q] = dn.t0d + dn.t1d;
    };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        // one query, one piece at a time.  S: the fourteen sums -- segment 0's S_a, S_j, S_xd, S_vd, S_ad, S_jd, segment 1's, then the own
        // duration0's and duration1's dotted end terms
        auto query = [&](int q, double lo_q, double hi_q, double dl_q, double lo_in, double hi_in, double dl_in, double g0_in, double g1_in,
                         double g2_in, double *S, double &lo_b, double &hi_b, double &dl_b) {
            const double d0v = L.h.d0[q], d0o = L.o.d0[q], Tv = L.Tv[q], To = L.To[q];
            const TrackWindow win = track_window<true>(SIDE ? d0o : d0v, SIDE ? To : Tv, SIDE ? d0v : d0o, SIDE ? Tv : To, lo_q, hi_q, dl_q);
            // ok: of the query as given; one without an answer counts with gradients and query tangents of zero
            const double g0 = win.ok ? g0_in : 0.0, g1 = win.ok ? g1_in : 0.0, g2 = win.ok ? g2_in : 0.0;
            const double dl_d = win.ok ? dl_in : 0.0;
            // the tangent of a piece end, by where it came from (k_tracking_jvp's)
            const double d0vd = L.h.d0_dot[q], d0od = L.o.d0_dot[q];
            const double d0Ad = SIDE ? d0od : d0vd, kBd = dl_d + (SIDE ? d0vd : d0od);
            const double ad = win.ok ? (win.cls_a == kPtLo ? lo_in : (win.cls_a == kPtStart ? dl_in : 0.0)) : 0.0;
            const double bd = win.cls_b == kPtHi ? (win.ok ? hi_in : 0.0)
                                                 : (win.cls_b == kPtEndA ? (SIDE ? L.Tod[q] : L.Tvd[q]) : dl_d + (SIDE ? L.Tvd[q] : L.Tod[q]));
            auto tangent = [&](int cls) { return cls == kEndA ? ad : (cls == kEndB ? bd : (cls == kEndKnotA ? d0Ad : kBd)); };
            double bar_a = 0.0, bar_b = 0.0, dl = 0.0, carry = 0.0;
            double &own0 = S[12];
            auto route = [&](int cls, double v) {
                bar_b += cls == kEndB ? v : 0.0;
                if (SIDE == 0) {
                    bar_a += cls == kEndA ? v : 0.0;
                    own0 += cls == kEndKnotA ? v : 0.0;
                    dl += cls == kEndKnotB ? v : 0.0;
                } else {
                    own0 += cls == kEndKnotB ? v : 0.0;
                }
            };
            track_pieces(win, [&](const TrackPiece &p) {
                const int seg_v = SIDE ? p.seg_b : p.seg_a, seg_o = SIDE ? p.seg_a : p.seg_b;
                const SegmentConst cv{L.x0[seg_v][q], L.h.c[seg_v][0][q], L.h.c[seg_v][3][q], L.h.c[seg_v][4][q], 0.0, 0.0};
                const SegmentConst tv{L.x0d[seg_v][q], L.h.t[seg_v][0][q], L.h.t[seg_v][3][q], L.h.t[seg_v][4][q], 0.0, 0.0};
                const SegmentConst co = eval_const(L.o.c, seg_o, q), to = eval_const(L.o.t, seg_o, q);
                const TrackState t = track_state(SIDE ? co : cv, SIDE ? cv : co, p);
                const double cd = tangent(p.cls_c), ed = tangent(p.cls_e);
                const double dsA = cd - (p.seg_a ? d0Ad : 0.0), dsB = cd - (p.seg_b ? kBd : dl_d), wd = ed - cd;
                // each side's own (vel, acc, jrk0) along the direction, and the tangent of the piece's state at fixed u
                double XAd, VAd, AAd, XBd, VBd, ABd;
                local_state(SIDE ? to : tv, p.sA, XAd, VAd, AAd);
                local_state(SIDE ? tv : to, p.sB, XBd, VBd, ABd);
                const double JAd = SIDE ? to.jrk0 : tv.jrk0, JBd = SIDE ? tv.jrk0 : to.jrk0;
                XAd += t.VA * dsA; VAd += t.AA * dsA; AAd += t.JA * dsA;
                XBd += t.VB * dsB; VBd += t.AB * dsB; ABd += t.JB * dsB;
                TrackState td;
                td.X = XAd - XBd; td.V = VAd - VBd; td.A = AAd - ABd; td.J = JAd - JBd;
                const double w = p.w, w2 = w * (w * 0.5), w3 = w2 * (w * (1.0 / 3.0));
                const double Dw = piece_end_gap(t, w), Vw = piece_end_rate(t, w), Aw = t.A + w * t.J;
                const double Ddw = piece_end_gap(td, w), Vdw = piece_end_rate(td, w);
                // the gradients on the tangent of the piece's state, (Xb, Vb, Ab, Jb), and their derivatives along the direction
                double Xb = g0 * w, Vb = g0 * w2, Ab = g0 * w3, Jb = g0 * (w3 * (w * 0.25));
                double Xbd = g0 * wd, Vbd = g0 * (w * wd), Abd = g0 * (w2 * wd), Jbd = g0 * (w3 * wd);
                {
                    double E0, E1, E2, E3;
                    gap_moments(t, w, E0, E1, E2, E3);
                    const double h = 2.0 * g1;
                    Xb += h * E0; Vb += h * E1; Ab += g1 * E2; Jb += g1 * (E3 * (1.0 / 3.0));
                    gap_moments(td, w, E0, E1, E2, E3);
                    const double e = Dw * wd;
                    E0 += e; E1 += w * e; E2 += (w * w) * e; E3 += (w * w * w) * e;
                    Xbd += h * E0; Vbd += h * E1; Abd += g1 * E2; Jbd += g1 * (E3 * (1.0 / 3.0));
                }
                {
                    double Q0, Q1, Q2;
                    rate_moments(t, w, Q0, Q1, Q2);
                    const double h = 2.0 * g2;
                    Vb += h * Q0; Ab += h * Q1; Jb += g2 * Q2;
                    rate_moments(td, w, Q0, Q1, Q2);
                    const double e = Vw * wd;
                    Q0 += e; Q1 += w * e; Q2 += (w * w) * e;
                    Vbd += h * Q0; Abd += h * Q1; Jbd += g2 * Q2;
                }
                // the launch's own side: the reverse rule's weights at its local start and their derivatives; B enters the gap with a minus
                {
                    const double s = SIDE ? p.sB : p.sA, sd = SIDE ? dsB : dsA, h2 = s * (s * 0.5), h3 = h2 * (s * (1.0 / 3.0));
                    const double W1 = Xb * s + Vb, W2 = Xb * h2 + Vb * s + Ab, W3 = Xb * h3 + Vb * h2 + Ab * s + Jb;
                    const double U[6] = {W2, W3, Xbd, (Xbd * s + Vbd) + Xb * sd, (Xbd * h2 + Vbd * s + Abd) + W1 * sd,
                                         (Xbd * h3 + Vbd * h2 + Abd * s + Jbd) + W2 * sd};
#pragma unroll
                    for (int f = 0; f < 6; ++f) {
                        const double Uf = SIDE ? -U[f] : U[f];
                        S[f] += seg_v ? 0.0 : Uf;
                        S[6 + f] += seg_v ? Uf : 0.0;
                    }
                }
                const double Fd = (g0 + (2.0 * g1) * Dw) * (Ddw + Vw * wd) + ((2.0 * g2) * Vw) * (Vdw + Aw * wd);
                const double PAd = (Xbd * t.VA + Vbd * t.AA + Abd * t.JA) + (Xb * VAd + Vb * AAd + Ab * JAd);
                const double PBd = (Xbd * t.VB + Vbd * t.AB + Abd * t.JB) + (Xb * VBd + Vb * ABd + Ab * JBd);
                // ds_A = dc - doff_A, ds_B = dc - doff_B, dw = de - dc: the reverse rule's routing, of the dotted terms
                route(p.cls_c, carry + ((PAd - PBd) - Fd));
                carry = Fd;
                if (SIDE == 0) {
                    own0 -= p.seg_a ? PAd : 0.0;
                    dl += PBd;
                } else {
                    own0 += p.seg_b ? PBd : 0.0;
                }
            });
            route(kEndB, carry);
            const bool own_end = win.cls_b == (SIDE ? kPtEndB : kPtEndA);
            S[12] += own_end ? bar_b : 0.0;
            S[13] += own_end ? bar_b : 0.0;
            if (SIDE == 0) {
                lo_b = win.cls_a == kPtLo ? bar_a : 0.0;
                hi_b = win.cls_b == kPtHi ? bar_b : 0.0;
                dl_b = (dl + (win.cls_a == kPtStart ? bar_a : 0.0)) + (win.cls_b == kPtEndB ? bar_b : 0.0);
            } else {
                lo_b = hi_b = dl_b = 0.0;
            }
        };
        // (a pair's two queries one after the other, each with its own 8-byte loads and stores, as in k_tracking_vjp)
        reduce_rows<14>(opaque_uniform(G), here, p_first, k, [&](int q, size_t at, bool two, double *S) {
            const double inf = __builtin_inf();
#pragma nounroll
            for (int second = 0; second < (two ? 2 : 1); ++second) {
                const size_t el = opaque_index(at + second);
                double lo_b, hi_b, dl_b;
                query(q, lo ? lo[el] : -inf, hi ? hi[el] : inf, delay ? delay[el] : 0.0, lo_dot ? lo_dot[el] : 0.0, hi_dot ? hi_dot[el] : 0.0,
                      delay_dot ? delay_dot[el] : 0.0, g.p[0] ? g.p[0][el] : 0.0, g.p[1] ? g.p[1][el] : 0.0, g.p[2] ? g.p[2][el] : 0.0, S, lo_b, hi_b,
                      dl_b);
                if (SIDE == 0) {
                    if (lo_bar_dot) lo_bar_dot[el] = lo_b;
                    if (hi_bar_dot) hi_bar_dot[el] = hi_b;
                    if (delay_bar_dot) delay_bar_dot[el] = dl_b;
                }
            }
        }, [&](int q, const double *S) {
            SegmentBar s0 = segment_chain_dot(L.h, 0, q, S, S + 3);
            SegmentBar s1 = segment_chain_dot(L.h, 1, q, S + 6, S + 9);
            s0.x0 += S[2];
            s1.x0 += S[8];
            route_bars(L.h.bar, q, s0, s1, s0.h + S[12], s1.h + S[13]);
            // a pair either of whose splines is under the NaN rule: all eight, also those that the other spline's NaN constants do not
            // reach (a segment of the own spline that no piece selects)
            if (L.Tv[q] != L.Tv[q] || L.To[q] != L.To[q]) {
#pragma unroll
                for (int f = 0; f < 8; ++f) L.h.bar[f][q] = quiet_nan();
            }
        });
        write_bars(L.h.bar, bar, p_first, here);
    });
}

// ---- when two splines meet: the first time the gap reaches a level (rp_trajectory_meeting) ----
// The inverse of section 18's gap, as the crossing is the evaluator's.  D, the common domain, the clamped window [a, b], the knots and the
// pieces are gap_query's; each piece is cut at its candidate roots of the relative velocity (gap_query's tests, the smaller first; a root
// that is no candidate leaves a sub-piece of length zero at the breakpoint before it), which leaves nine monotone sub-pieces between ten
// breakpoints in time order: a, roots, knot, roots, knot, roots, b (a knot outside [a, b]: the end it is clamped to).  Every breakpoint's
// gap is gap_at there, once: the end of one sub-piece and the start of the next are the same number, so a level between D(a) and D(b) is
// held by some sub-piece.  A query takes the first sub-piece whose end values hold its level between them; a level equal to the value at
// the sub-piece's start is that breakpoint with its own bits; otherwise bracket_search solves D(c + u) = level in the piece's local form --
// (X, V, A, J) the differences of the two selected segments at the piece's start c, as track_state forms them, u from the sub-piece's
// start - c to its end - c, the stopping width 2 ulp of the sub-piece's later end as a time on A's clock -- and the time is c + u, kept
// inside the sub-piece.  The closing velocity that comes back is the evaluators' at that time.  The local form, not two eval_query calls
// per trip: the search then holds five numbers instead of reading ten per trip from LDS behind two selects.  The two queries of a pair run
// one after the other: each search's trip count is its own.
__device__ __forceinline__ void meeting_query(const GapLds &L, int q, double level, double lo, double hi, double delay, double &time,
                                              double &relvel)
{
    const double kA = L.a.d0[q], kB = delay + L.b.d0[q], TA = L.Ta[q], EB = delay + L.Tb[q];
    const double S = delay > 0.0 ? delay : 0.0, E = EB < TA ? EB : TA;      // gap_query's domain, window and knots
    const double a = lo > S ? lo : (lo != lo ? lo : S), b = hi < E ? hi : (hi != hi ? hi : E);
    const bool ok = a <= b && finite_(delay) && EB == EB;
    const bool b_first = kB < kA;
    bool found = false;
    double t_lo = 0.0, t_hi = 0.0, g_lo = 0.0, g_hi = 0.0, c_at = 0.0;      // the sub-piece taken, its end values minus the level, its piece's start
    double c = a, t_prev = a, v_prev = gap_at(L, q, a, delay);
    auto breakpoint = [&](bool real, double t) {
        const double v = gap_at(L, q, t, delay);
        const double t_next = real ? t : t_prev, v_next = real ? v : v_prev;
        const bool holds = (v_prev <= level && level <= v_next) || (v_next <= level && level <= v_prev);      // a NaN fails
        if (ok && !found && holds) {
            found = true;
            t_lo = t_prev; t_hi = t_next;
            g_lo = v_prev - level; g_hi = v_next - level;
            c_at = c;
        }
        t_prev = t_next;
        v_prev = v_next;
    };
#pragma nounroll
    for (int piece = 0; piece < 3; ++piece) {
        const double knot = (piece == 0) == b_first ? kB : kA;
        const double e = piece == 2 ? b : (knot < a ? a : (knot > b ? b : knot));
        const int seg_a = kA <= c, seg_b = kB <= c;
        double vel_a, acc_a, jrk_a, vel_b, acc_b, jrk_b, r0, r1;
        local_motion(L.a, seg_a, q, seg_a ? c - kA : c, vel_a, acc_a, jrk_a);
        local_motion(L.b, seg_b, q, seg_b ? c - kB : c - delay, vel_b, acc_b, jrk_b);
        velocity_roots(vel_a - vel_b, acc_a - acc_b, jrk_a - jrk_b, r0, r1);
        const double length = e - c, t0 = c + r0, t1 = c + r1;
        const bool in0 = ok && r0 > 0.0 && r0 < length && a < t0 && t0 < b, in1 = ok && r1 > 0.0 && r1 < length && a < t1 && t1 < b;
        const bool swap = in1 && (!in0 || r1 < r0);
        breakpoint(swap ? in1 : in0, swap ? t1 : t0);
        breakpoint(swap ? in0 : in1, swap ? t0 : t1);
        breakpoint(true, e);
        c = e;
    }
    time = relvel = quiet_nan();
    if (!found) return;
    double t = t_lo;
    if (g_lo != 0.0) {
        TrackPiece p;
        p.seg_a = kA <= c_at;
        p.seg_b = kB <= c_at;
        p.sA = p.seg_a ? c_at - kA : c_at;
        p.sB = p.seg_b ? c_at - kB : c_at - delay;
        const TrackState st = track_state(eval_const(L.a.c, p.seg_a, q), eval_const(L.b.c, p.seg_b, q), p);
        const double u = bracket_search(st.X, st.V, st.A, st.J, level, t_lo - c_at, t_hi - c_at, g_lo, g_hi, kCrossTol * t_hi);
        t = c_at + u;
        t = t < t_lo ? t_lo : (t > t_hi ? t_hi : t);
    }
    double pos, vel_a, vel_b, acc;
    eval_query(L.a, q, t, pos, vel_a, acc);
    eval_query(L.b, q, t - delay, pos, vel_b, acc);
    time = t;
    relvel = vel_a - vel_b;
}

__global__ void __launch_bounds__(kTrajBlock)
k_meeting(FromArrays a, FromArrays b, size_t n, size_t k, int P, const double *__restrict__ level, const double *__restrict__ lo,
          const double *__restrict__ hi, const double *__restrict__ delay, double *__restrict__ time, double *__restrict__ relvel)
{
    __shared__ GapLds L;
    auto stage_problem = [&](int q, size_t i) {
        Knots ka = a.load(i), kb = b.load(i);
        ka.check();
        kb.check();
        stage_eval(L.a, q, ka);
        stage_eval(L.b, q, kb);
        L.Ta[q] = ka.t0 + ka.t1;
        L.Tb[q] = kb.t0 + kb.t1;
    };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double pa = 0.0, pb = 0.0, la, lb, ha, hb, da = 0.0, db = 0.0, ta, tb, va, vb;
            if (level) load_pair(level, e_first + e, two, pa, pb);
            load_window(lo, hi, e_first + e, two, la, lb, ha, hb);
            if (delay) load_pair(delay, e_first + e, two, da, db);
            meeting_query(L, qa, pa, la, ha, da, ta, va);
            if (two) meeting_query(L, qb, pb, lb, hb, db, tb, vb); else { tb = ta; vb = va; }
            store_pair(time, e_first + e, ta, tb, two);
            if (relvel) store_pair(relvel, e_first + e, va, vb, two);
        });
    });
}

// ---- how close two vehicles moving in D axes get: the least squared distance over a window (rp_trajectory_separation; DESIGN.md section
// 24) ----
// Vehicle A is D splines, one per axis, vehicle B likewise, B on a clock that starts `delay` after A's; D_c(t) = pos_Ac(t) - pos_Bc(t - delay)
// and f(t) = the sum over the axes of D_c(t)^2 on the common domain [S, E], S = delay > 0 ? delay : +0.0, E the smallest of the 2 D ends T_Ac and
// delay + T_Bc (A's before B's and a lower axis first among equals).  A query clamps its window to [a, b] as gap_query does and walks 2 D + 1
// pieces without sorting the 2 D knots k_Ac = duration0_Ac, k_Bc = delay + duration0_Bc: a piece ends at the smallest knot greater than its
// start and smaller than b, else at b (after which the remaining pieces have length zero).  On a piece with start c every axis' (X, V, A, J) is
// track_state's, and with u = t - c
//     g(u) = f'(u) / 2 = the sum of D_c(u) D_c'(u)
// is a quintic in u whose six coefficients are plain products and sums of those 4 D numbers.  Its roots with a change of sign are isolated by
// the derivative chain: the roots of g''' in closed form (velocity_breaks: padded to two breakpoints in [0, length]) bracket those of g'',
// those bracket the roots of g', those the roots of g.  Between two neighbouring breakpoints a polynomial whose end values differ in sign is
// solved by poly_search -- bracket_search's shape: Newton steps kept inside the bracket, bisection where a step leaves it or fails to halve the
// step before last, the point of smallest |p| looked at, kSepTrips trips at most -- and the end values are computed once, the end of one
// bracket being the start of the next.  No step divides by a leading coefficient: a polynomial of lower degree, or one that is zero (the
// follower without a delay), has no change of sign.  A bracket without one leaves NaN, which the next level takes as a bracket of length zero.
// Candidates in time order: a; per piece the roots of g strictly inside (0, length) and, as times c + u, strictly inside (a, b), then the
// knot that ends the piece; b.  Every candidate's value is sep_at: the sum in axis order of the squares of eval_query(A_c, t) -
// eval_query(B_c, t - delay); the walk is Extreme::take's for the minimum alone (strict: the earliest among equals, a NaN never) and the
// time that comes back carries its candidate's own bits.  Selects only outside poly_search's loop; the pieces are a loop of 2 D + 1 trips and
// the two queries of a pair a loop of two, both kept as loops, and so are the loops over the axes in sep_at and in the coefficient sum:
// unrolled, the LDS reads of all axes are in flight together and D = 2 takes 149 VGPRs; kept, one axis' numbers are live at a time (125,
// 126, 130 VGPRs for D = 1, 2, 3).  `trips` counts the searches' trips for the host-side cut of this code (tests/checks); the kernel drops
// it.  The block's first P threads leave per problem the 2 D splines' evaluator constants and total times: 20 KiB of LDS per axis.
constexpr int kSepTrips = 64;      // bisection alone reaches 2 ulp of any double bracket in ~53

template <int D> struct SepLds {
    EvalLds a[D], b[D];
    double Ta[D][kTrajProblems], Tb[D][kTrajProblems];
};

// p[0] + p[1] u + ... + p[N - 1] u^(N - 1) and its derivative, by Horner's rule
template <int N> __device__ __forceinline__ double poly_at(const double (&p)[N], double u)
{
    double v = p[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 0; --i) v = p[i] + u * v;
    return v;
}

template <int N> __device__ __forceinline__ double poly_slope(const double (&p)[N], double u)
{
    double v = (double)(N - 1) * p[N - 1];
#pragma unroll
    for (int i = N - 2; i >= 1; --i) v = (double)i * p[i] + u * v;
    return v;
}

// the root of p in the bracket [lo, hi] whose ends leave p_lo != 0 and p_hi of the other sign: the point of smallest |p| looked at
template <int N>
__device__ __forceinline__ double poly_search(const double (&p)[N], double lo, double hi, double p_lo, double p_hi, double tol, int &trips)
{
    const bool up = p_lo < 0.0;
    double width = hi - lo;
    double best = abs_(p_hi) < abs_(p_lo) ? hi : lo, best_p = min_(abs_(p_lo), abs_(p_hi));
    double s = lo + width * (p_lo * rcp_<double>(p_lo - p_hi));      // the secant point of the bracket
    if (!(s > lo && s < hi)) s = lo + 0.5 * width;
    double dx_old = width, dx = width;
    for (int trip = 0; trip < kSepTrips; ++trip) {
        const double g = poly_at(p, s), v = poly_slope(p, s);
        ++trips;
        if (abs_(g) < best_p) { best_p = abs_(g); best = s; }
        if (g == 0.0) break;
        if ((g < 0.0) == up) lo = s; else hi = s;
        width = hi - lo;
        if (!(width > tol)) break;
        const double step = g * rcp_<double>(v);      // v == 0: infinite, outside
        double next = s - step;
        if (!(next > lo && next < hi && 2.0 * abs_(step) <= abs_(dx_old))) next = lo + 0.5 * width;
        dx_old = dx;
        dx = next - s;
        if (!(abs_(dx) > tol)) break;
        s = next;
    }
    return best;
}

// one level of the chain: the roots of p in (0, len] between the breakpoints brk (in order, NaN: none), one per bracket (NaN: none)
template <int N, int M>
__device__ __forceinline__ void roots_between(const double (&p)[N], const double (&brk)[M], double len, double tol, double (&out)[M + 1], int &trips)
{
    double lo = 0.0, p_lo = p[0];
#pragma unroll
    for (int j = 0; j <= M; ++j) {
        const double mid = brk[j < M ? j : M - 1];
        const double hi = j < M ? (mid == mid ? mid : lo) : len;
        const double p_hi = poly_at(p, hi);
        const bool cross = (p_lo < 0.0 && p_hi >= 0.0) || (p_lo > 0.0 && p_hi <= 0.0);      // a NaN fails
        double r = quiet_nan();
        if (cross) r = p_hi == 0.0 ? hi : poly_search(p, lo, hi, p_lo, p_hi, tol, trips);
        out[j] = r;
        lo = hi;
        p_lo = p_hi;
    }
}

template <int D> __device__ __forceinline__ double sep_at(const SepLds<D> &L, int q, double t, double delay)
{
    double sum = 0.0;      // (0.0 + x * x is x * x bit for bit)
#pragma nounroll
    for (int x = 0; x < D; ++x) {      // a loop that is kept: one axis' numbers live at a time
        double pa, pb, vel, acc;
        eval_query(L.a[x], q, t, pa, vel, acc);
        eval_query(L.b[x], q, t - delay, pb, vel, acc);
        const double gap = pa - pb;
        sum = sum + gap * gap;
    }
    return sum;
}

template <int D>
__device__ __forceinline__ void separation_query(const SepLds<D> &L, int q, double lo, double hi, double delay, double &value, double &time,
                                                 int &trips)
{
    double E = __builtin_inf();
    bool whole = true;      // none of the 2 D splines under the NaN rule
#pragma unroll
    for (int x = 0; x < D; ++x) {
        const double TA = L.Ta[x][q];
        whole = whole && TA == TA;
        E = TA < E ? TA : E;
    }
#pragma unroll
    for (int x = 0; x < D; ++x) {
        const double EB = delay + L.Tb[x][q];
        whole = whole && EB == EB;
        E = EB < E ? EB : E;
    }
    const double S = delay > 0.0 ? delay : 0.0;
    const double a = lo > S ? lo : (lo != lo ? lo : S), b = hi < E ? hi : (hi != hi ? hi : E);      // clamp_window's rule from S on
    const bool ok = a <= b && finite_(delay) && whole;
    double best_v = quiet_nan(), best_t = quiet_nan();
    auto take = [&](bool on, double t) {
        const double v = sep_at(L, q, t, delay);
        const bool less = on && (v < best_v || (best_v != best_v && v == v));
        best_v = less ? v : best_v;
        best_t = less ? t : best_t;
    };
    take(ok, a);
    double c = a;
#pragma nounroll
    for (int piece = 0; piece < 2 * D + 1; ++piece) {
        double e = b;
#pragma unroll
        for (int x = 0; x < D; ++x) {
            const double kA = L.a[x].d0[q], kB = delay + L.b[x].d0[q];
            e = kA > c && kA < e ? kA : e;
            e = kB > c && kB < e ? kB : e;
        }
        const bool knot = ok && e < b;
        double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
#pragma nounroll
        for (int x = 0; x < D; ++x) {
            const double kA = L.a[x].d0[q], kB = delay + L.b[x].d0[q];
            TrackPiece p;
            p.seg_a = kA <= c;
            p.seg_b = kB <= c;
            p.sA = p.seg_a ? c - kA : c;
            p.sB = p.seg_b ? c - kB : c - delay;
            const TrackState st = track_state(eval_const(L.a[x].c, p.seg_a, q), eval_const(L.b[x].c, p.seg_b, q), p);
            const double p0 = st.X, p1 = st.V, p2 = st.A * 0.5, p3 = st.J * (1.0 / 6.0);      // D_c(u)
            const double q0 = st.V, q1 = st.A, q2 = st.J * 0.5;                                // D_c'(u)
            const double t[6] = {p0 * q0, p0 * q1 + p1 * q0, (p0 * q2 + p1 * q1) + p2 * q0, (p1 * q2 + p2 * q1) + p3 * q0, p2 * q2 + p3 * q1,
                                 p3 * q2};
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = g[i] + t[i];
        }
        const double len = e - c, tol = kCrossTol * e;
        const double g1[5] = {g[1], 2.0 * g[2], 3.0 * g[3], 4.0 * g[4], 5.0 * g[5]};
        const double g2[4] = {2.0 * g[2], 6.0 * g[3], 12.0 * g[4], 20.0 * g[5]};
        double r3[2], r2[3], r1[4], r0[5];
        velocity_breaks(6.0 * g[3], 24.0 * g[4], 120.0 * g[5], len, r3[0], r3[1]);      // g''' = 6 g3 + 24 g4 u + 60 g5 u^2
        roots_between(g2, r3, len, tol, r2, trips);
        roots_between(g1, r2, len, tol, r1, trips);
        roots_between(g, r1, len, tol, r0, trips);
#pragma unroll
        for (int j = 0; j < 5; ++j) {
            const double u = r0[j], t = c + u;
            take(ok && u > 0.0 && u < len && a < t && t < b, t);
        }
        take(knot, e);
        c = e;
    }
    take(ok, b);
    value = best_v;
    time = best_t;
}

template <int D> struct SepSplines { FromArrays a[D], b[D]; };      // a pair entry's tables: vehicle A's D splines and vehicle B's
template <int D> struct FleetSplines { FromArrays v[D]; };          // a fleet entry's: vehicle v of scene s at s m + v of every array

// The one staging of a pair (sections 24-28): problem ia of a's D splines as vehicle A and problem ib of b's as vehicle B into place q,
// under the NaN rule, each axis' evaluator constants and total time.
template <int D>
__device__ __forceinline__ void stage_vehicles(SepLds<D> &L, int q, const FromArrays (&a)[D], size_t ia, const FromArrays (&b)[D], size_t ib)
{
#pragma unroll
    for (int x = 0; x < D; ++x) {
        Knots ka = a[x].load(ia), kb = b[x].load(ib);
        ka.check();
        kb.check();
        stage_eval(L.a[x], q, ka);
        stage_eval(L.b[x], q, kb);
        L.Ta[x][q] = ka.t0 + ka.t1;
        L.Tb[x][q] = kb.t0 + kb.t1;
    }
}

// The one decode of a fleet launch's problem p, staged by thread q of its trip, into (scene, i, j) (section 26: one 64-bit division for
// the trip's first scene, 32-bit ones from there), and the staging of vehicles i and j of that scene as A and B.
template <int D>
__device__ __forceinline__ void stage_fleet_pair(SepLds<D> &L, int q, const FleetSplines<D> &in, unsigned m, unsigned pairs, size_t p)
{
    const size_t p_first = p - (size_t)q, s_first = p_first / pairs;
    const unsigned r = (unsigned)(p_first - s_first * pairs) + (unsigned)q;      // < pairs + kTrajProblems
    const size_t s = s_first + r / pairs;
    unsigned i, j;
    fleet_pair(r % pairs, m, i, j);
    stage_vehicles(L, q, in.v, s * m + i, in.v, s * m + j);
}

template <int D>
__global__ void __launch_bounds__(kTrajBlock) 
k_separation(SepSplines<D> in, size_t n, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi,
             const double *__restrict__ delay, double *__restrict__ value, double *__restrict__ time)
{
    __shared__ SepLds<D> L;
    auto stage_problem = [&](int q, size_t i) { stage_vehicles(L, q, in.a, i, in.b, i); };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double la, lb, ha, hb, da = 0.0, db = 0.0, va = 0.0, vb = 0.0, ta = 0.0, tb = 0.0;
            load_window(lo, hi, e_first + e, two, la, lb, ha, hb);
            if (delay) load_pair(delay, e_first + e, two, da, db);
#pragma nounroll
            for (int half = 0; half < (two ? 2 : 1); ++half) {      // one after the other: each query's searches have their own trip counts
                double v, t;
                int trips = 0;
                separation_query(L, half ? qb : qa, half ? lb : la, half ? hb : ha, half ? db : da, v, t, trips);
                va = half ? va : v; ta = half ? ta : t;
                vb = half ? v : vb; tb = half ? t : tb;
            }
            if (value) store_pair(value, e_first + e, va, vb, two);
            if (time) store_pair(time, e_first + e, ta, tb, two);
        });
    });
}

// ---- the closest approach of every pair of a fleet (rp_trajectory_fleet_separation) ----
// n scenes of m vehicles on one clock, vehicle v of scene s at s m + v of every array.  The launch's problems are the n m (m - 1) / 2 (scene,
// pair) combinations in output order: the staging thread of problem p decodes (s, i, j) (fleet_index.h) and stages vehicle i as k_separation
// stages A and vehicle j as it stages B -- L2 takes the m - 1 reads of a vehicle; no pair-expanded array exists.  A query finds its scene's
// window, lo and hi n x k, with plain 8-byte loads at s k + its column.  The scene of a problem is not kept in LDS: 4 x 40 KiB of SepLds<2>
// are all of a CU's 160 KiB, and any array next to it costs D = 2 its fourth block (the compiler then also answers the four-wave hint with
// 133 VGPRs).  Instead one 64-bit division per trip gives the trip's first (scene, pair), and place q's are a 32-bit division on from there.
// Every query is separation_query with a delay of 0.0: k_separation's bits for the gathered pair with a null delay.  Without the hint the
// allocator takes 127 / 133 / 142 VGPRs.
template <int D>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(D == 3 ? 2 : 4, 8)))
k_fleet(FleetSplines<D> in, size_t problems, unsigned m, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi,
        double *__restrict__ value, double *__restrict__ time)
{
    __shared__ SepLds<D> L;
    const unsigned pairs = fleet_pair_count(m);
    auto stage_problem = [&](int q, size_t p) { stage_fleet_pair(L, q, in, m, pairs, p); };
    for_each_trip(problems, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k, s_first = p_first / pairs;
        const unsigned r_first = (unsigned)(p_first - s_first * pairs);
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            const double inf = __builtin_inf();
            const size_t sa = s_first + (r_first + (unsigned)qa) / pairs, sb = s_first + (r_first + (unsigned)qb) / pairs;
            const size_t wa = sa * k + (e - (size_t)qa * k);                            // the scene's row, the query's column
            const size_t wb = two ? sb * k + (e + 1 - (size_t)qb * k) : wa;
            const double la = lo ? lo[wa] : -inf, lb = lo ? lo[wb] : -inf, ha = hi ? hi[wa] : inf, hb = hi ? hi[wb] : inf;
            double va = 0.0, vb = 0.0, ta = 0.0, tb = 0.0;
#pragma nounroll
            for (int half = 0; half < (two ? 2 : 1); ++half) {      // as k_separation: each query's searches have their own trip counts
                double v, t;
                int trips = 0;
                separation_query(L, half ? qb : qa, half ? lb : la, half ? hb : ha, 0.0, v, t, trips);
                va = half ? va : v; ta = half ? ta : t;
                vb = half ? v : vb; tb = half ? t : tb;
            }
            if (value) store_pair(value, e_first + e, va, vb, two);
            if (time) store_pair(time, e_first + e, ta, tb, two);
        });
    });
}

// ---- the closest approach of every vehicle of one fleet to every vehicle of another (rp_trajectory_cross_separation) ----
// n scenes of m_a vehicles of fleet A and m_b of fleet B on one clock: A's arrays hold n m_a values, vehicle v of scene s at s m_a + v, B's
// n m_b, at s m_b + v.  The launch's problems are the n m_a m_b (scene, pair) combinations in output order, pair r = (r / m_b, r % m_b)
// (fleet_index.h): k_fleet with two tables and a rectangle where it has one table and a triangle.  The scene is not kept in LDS, the windows
// are n x k and read at s k + the column, and every query is separation_query with a delay of 0.0: k_separation's bits for the gathered pair
// with a null delay.  pairs <= 2^30, so r_first + a place stays inside 32 bits.
template <int D> struct CrossSplines { FromArrays a[D], b[D]; };      // a cross entry's tables: fleet A's D splines and fleet B's

// stage_fleet_pair's decode for the rectangle: one 64-bit division for the trip's first scene, 32-bit ones from there
template <int D>
__device__ __forceinline__ void stage_cross_pair(SepLds<D> &L, int q, const CrossSplines<D> &in, unsigned m_a, unsigned m_b, unsigned pairs, size_t p)
{
    const size_t p_first = p - (size_t)q, s_first = p_first / pairs;
    const unsigned r = (unsigned)(p_first - s_first * pairs) + (unsigned)q;      // < pairs + kTrajProblems
    const size_t s = s_first + r / pairs;
    unsigned i, j;
    cross_pair(r % pairs, m_b, i, j);
    stage_vehicles(L, q, in.a, s * m_a + i, in.b, s * m_b + j);
}

template <int D>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(D == 3 ? 2 : 4, 8)))
k_versus(CrossSplines<D> in, size_t problems, unsigned m_a, unsigned m_b, size_t k, int P, const double *__restrict__ lo,
         const double *__restrict__ hi, double *__restrict__ value, double *__restrict__ time)
{
    __shared__ SepLds<D> L;
    const unsigned pairs = cross_pair_count(m_a, m_b);
    auto stage_problem = [&](int q, size_t p) { stage_cross_pair(L, q, in, m_a, m_b, pairs, p); };
    for_each_trip(problems, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k, s_first = p_first / pairs;
        const unsigned r_first = (unsigned)(p_first - s_first * pairs);
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            const double inf = __builtin_inf();
            const size_t sa = s_first + (r_first + (unsigned)qa) / pairs, sb = s_first + (r_first + (unsigned)qb) / pairs;
            const size_t wa = sa * k + (e - (size_t)qa * k);                            // the scene's row, the query's column
            const size_t wb = two ? sb * k + (e + 1 - (size_t)qb * k) : wa;
            const double la = lo ? lo[wa] : -inf, lb = lo ? lo[wb] : -inf, ha = hi ? hi[wa] : inf, hb = hi ? hi[wb] : inf;
            double va = 0.0, vb = 0.0, ta = 0.0, tb = 0.0;
#pragma nounroll
            for (int half = 0; half < (two ? 2 : 1); ++half) {      // as k_separation: each query's searches have their own trip counts
                double v, t;
                int trips = 0;
                separation_query(L, half ? qb : qa, half ? lb : la, half ? hb : ha, 0.0, v, t, trips);
                va = half ? va : v; ta = half ? ta : t;
                vb = half ? v : vb; tb = half ? t : tb;
            }
            if (value) store_pair(value, e_first + e, va, vb, two);
            if (time) store_pair(time, e_first + e, ta, tb, two);
        });
    });
}

// ---- when two vehicles moving in D axes first come within a distance (rp_trajectory_contact) ----
// The inverse of section 24's squared distance f, as the meeting is the gap's.  The splines, the NaN rule, the domain, the clamped window
// [a, b], the knots, the unsorted walk of 2 D + 1 pieces and each piece's quintic g = f' / 2 with its sign-changing roots r0[0..4] are
// separation_query's, operation for operation.  A piece [c, e] is cut at those of its roots that are separation_query's candidates (a root
// that is none repeats the breakpoint before it: a sub-piece of length zero), which leaves six sub-pieces on which f is monotone.  Every
// breakpoint's value is sep_at there, once: f(a) before the walk, and the f(e) of one piece is the f(c) of the next, so a level between
// f(a) and f(b) is held by some sub-piece whatever the rounding.  A query takes the first sub-piece whose end values hold its level between
// them; a level equal to the value at the sub-piece's start is that breakpoint with its own bits; otherwise poly_search solves
//     h(u) = (F0 - level) + the sum of g_i (2 / (i + 1)) u^(i + 1) = 0,      F0 = the sum in axis order of X_c^2,
// f - level in the piece's local form, from the sub-piece's start - c to its end - c with the breakpoint values minus the level as the end
// values and the piece's stopping width; the time is c + u, kept inside the sub-piece.  The local form inside the search and the evaluator
// at its ends: meeting_query's reason.  The rate that comes back is f' at that time on the evaluators' outputs.  A query whose window,
// delay, level or splines make it NaN returns before the walk: no search runs for it.  The walk ends with the piece that holds the answer,
// and at a piece after the first that starts at b (length zero: its six sub-pieces repeat f(b), which the sub-piece before them has
// already been asked about); neither changes a bit (section 25 has the A/B).  One search site per piece: the six breakpoints select the
// sub-piece, the search follows them.
template <int D> __device__ __forceinline__ double sep_rate_at(const SepLds<D> &L, int q, double t, double delay)
{
    double sum = 0.0;
#pragma nounroll
    for (int x = 0; x < D; ++x) {
        double pa, pb, va, vb, acc;
        eval_query(L.a[x], q, t, pa, va, acc);
        eval_query(L.b[x], q, t - delay, pb, vb, acc);
        sum = sum + (pa - pb) * (va - vb);
    }
    return 2.0 * sum;
}

template <int D>
__device__ __forceinline__ void contact_query(const SepLds<D> &L, int q, double level, double lo, double hi, double delay, double &time,
                                              double &rate, int &trips)
{
    double E = __builtin_inf();
    bool whole = true;      // none of the 2 D splines under the NaN rule
#pragma unroll
    for (int x = 0; x < D; ++x) {
        const double TA = L.Ta[x][q];
        whole = whole && TA == TA;
        E = TA < E ? TA : E;
    }
#pragma unroll
    for (int x = 0; x < D; ++x) {
        const double EB = delay + L.Tb[x][q];
        whole = whole && EB == EB;
        E = EB < E ? EB : E;
    }
    const double S = delay > 0.0 ? delay : 0.0;
    const double a = lo > S ? lo : (lo != lo ? lo : S), b = hi < E ? hi : (hi != hi ? hi : E);      // clamp_window's rule from S on
    time = rate = quiet_nan();
    if (!(a <= b && finite_(delay) && finite_(level) && whole)) return;
    bool found = false;
    double t_found = 0.0;
    double c = a, f_c = sep_at(L, q, a, delay);
#pragma nounroll
    for (int piece = 0; piece < 2 * D + 1; ++piece) {
        if (found || (piece > 0 && !(c < b))) break;
        double e = b;
#pragma unroll
        for (int x = 0; x < D; ++x) {
            const double kA = L.a[x].d0[q], kB = delay + L.b[x].d0[q];
            e = kA > c && kA < e ? kA : e;
            e = kB > c && kB < e ? kB : e;
        }
        double g[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, F0 = 0.0;
#pragma nounroll
        for (int x = 0; x < D; ++x) {
            const double kA = L.a[x].d0[q], kB = delay + L.b[x].d0[q];
            TrackPiece p;
            p.seg_a = kA <= c;
            p.seg_b = kB <= c;
            p.sA = p.seg_a ? c - kA : c;
            p.sB = p.seg_b ? c - kB : c - delay;
            const TrackState st = track_state(eval_const(L.a[x].c, p.seg_a, q), eval_const(L.b[x].c, p.seg_b, q), p);
            const double p0 = st.X, p1 = st.V, p2 = st.A * 0.5, p3 = st.J * (1.0 / 6.0);      // D_c(u)
            const double q0 = st.V, q1 = st.A, q2 = st.J * 0.5;                                // D_c'(u)
            const double t[6] = {p0 * q0, p0 * q1 + p1 * q0, (p0 * q2 + p1 * q1) + p2 * q0, (p1 * q2 + p2 * q1) + p3 * q0, p2 * q2 + p3 * q1,
                                 p3 * q2};
#pragma unroll
            for (int i = 0; i < 6; ++i) g[i] = g[i] + t[i];
            F0 = F0 + p0 * p0;
        }
        const double len = e - c, tol = kCrossTol * e;
        const double g1[5] = {g[1], 2.0 * g[2], 3.0 * g[3], 4.0 * g[4], 5.0 * g[5]};
        const double g2[4] = {2.0 * g[2], 6.0 * g[3], 12.0 * g[4], 20.0 * g[5]};
        double r3[2], r2[3], r1[4], r0[5];
        velocity_breaks(6.0 * g[3], 24.0 * g[4], 120.0 * g[5], len, r3[0], r3[1]);      // g''' = 6 g3 + 24 g4 u + 60 g5 u^2
        roots_between(g2, r3, len, tol, r2, trips);
        roots_between(g1, r2, len, tol, r1, trips);
        roots_between(g, r1, len, tol, r0, trips);
        bool here = false;
        double t_lo = 0.0, t_hi = 0.0, f_lo = 0.0, f_hi = 0.0;      // the sub-piece taken and its end values
        double t_prev = c, f_prev = f_c;
#pragma unroll
        for (int j = 0; j < 6; ++j) {
            const double u = r0[j < 5 ? j : 4], t = j < 5 ? c + u : e;
            const bool real = j == 5 || (u > 0.0 && u < len && a < t && t < b);
            const double f = sep_at(L, q, t, delay);
            const double t_next = real ? t : t_prev, f_next = real ? f : f_prev;
            const bool holds = (f_prev <= level && level <= f_next) || (f_next <= level && level <= f_prev);      // a NaN fails
            const bool first = holds && !here;
            t_lo = first ? t_prev : t_lo; t_hi = first ? t_next : t_hi;
            f_lo = first ? f_prev : f_lo; f_hi = first ? f_next : f_hi;
            here = here || holds;
            t_prev = t_next;
            f_prev = f_next;
        }
        if (here) {
            double t = t_lo;
            if (f_lo != level) {
                const double h[7] = {F0 - level, g[0] * 2.0, g[1] * (2.0 / 2.0), g[2] * (2.0 / 3.0), g[3] * (2.0 / 4.0), g[4] * (2.0 / 5.0),
                                     g[5] * (2.0 / 6.0)};
                t = c + poly_search(h, t_lo - c, t_hi - c, f_lo - level, f_hi - level, tol, trips);
                t = t < t_lo ? t_lo : (t > t_hi ? t_hi : t);
            }
            found = true;
            t_found = t;
        }
        c = e;
        f_c = f_prev;
    }
    if (!found) return;
    time = t_found;
    rate = sep_rate_at(L, q, t_found, delay);
}

// Left to itself the allocator takes 132 / 142 / 141 VGPRs -- the level, F0 and the pair's second level more than k_separation carries -- which
// is three waves per SIMD for D = 1, 2 where k_separation has four; asked for four it fits 128 / 128 without scratch (section 25).
template <int D>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(D == 3 ? 3 : 4, 8)))
k_contact(SepSplines<D> in, size_t n, size_t k, int P, const double *__restrict__ level, const double *__restrict__ lo,
          const double *__restrict__ hi, const double *__restrict__ delay, double *__restrict__ time, double *__restrict__ rate)
{
    __shared__ SepLds<D> L;
    auto stage_problem = [&](int q, size_t i) { stage_vehicles(L, q, in.a, i, in.b, i); };
    for_each_trip(n, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k;
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double pa, pb, la, lb, ha, hb, da = 0.0, db = 0.0, ta = 0.0, tb = 0.0, ra = 0.0, rb = 0.0;
            load_pair(level, e_first + e, two, pa, pb);
            load_window(lo, hi, e_first + e, two, la, lb, ha, hb);
            if (delay) load_pair(delay, e_first + e, two, da, db);
#pragma nounroll
            for (int half = 0; half < (two ? 2 : 1); ++half) {      // one after the other: each query's searches have their own trip counts
                double t, r;
                int trips = 0;
                contact_query(L, half ? qb : qa, half ? pb : pa, half ? lb : la, half ? hb : ha, half ? db : da, t, r, trips);
                ta = half ? ta : t; ra = half ? ra : r;
                tb = half ? t : tb; rb = half ? r : rb;
            }
            store_pair(time, e_first + e, ta, tb, two);
            if (rate) store_pair(rate, e_first + e, ra, rb, two);
        });
    });
}

// ---- the first contact of every pair of a fleet (rp_trajectory_fleet_contact) ----
// k_fleet's staging and scene arithmetic around contact_query: the launch's problems are the n m (m - 1) / 2 (scene, pair) combinations in
// output order, the staging thread of problem p decodes (s, i, j) and stages vehicles i and j where they lie, and the scene of a problem is
// not kept in LDS (one 64-bit division per trip, 32-bit divisions from there: section 26).  A query's window ends are 8-byte loads at
// s k + its column.  The level, in units of squared distance, is either per scene (level_per_pair 0: n x k, read where the window
// ends are) or per pair (1: n x pairs x k, in the outputs' layout, read with load_pair as k_contact reads its level).  Every query is
// contact_query with a delay of 0.0: k_contact's bits for the gathered pair with a null delay.
template <int D>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(D == 3 ? 2 : 4, 8)))
k_encounter(FleetSplines<D> in, size_t problems, unsigned m, size_t k, int P, const double *__restrict__ level, int level_per_pair,
            const double *__restrict__ lo, const double *__restrict__ hi, double *__restrict__ time, double *__restrict__ rate)
{
    __shared__ SepLds<D> L;
    const unsigned pairs = fleet_pair_count(m);
    auto stage_problem = [&](int q, size_t p) { stage_fleet_pair(L, q, in, m, pairs, p); };
    for_each_trip(problems, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k, s_first = p_first / pairs;
        const unsigned r_first = (unsigned)(p_first - s_first * pairs);
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            const double inf = __builtin_inf();
            const size_t sa = s_first + (r_first + (unsigned)qa) / pairs, sb = s_first + (r_first + (unsigned)qb) / pairs;
            const size_t wa = sa * k + (e - (size_t)qa * k);                            // the scene's row, the query's column
            const size_t wb = two ? sb * k + (e + 1 - (size_t)qb * k) : wa;
            const double la = lo ? lo[wa] : -inf, lb = lo ? lo[wb] : -inf, ha = hi ? hi[wa] : inf, hb = hi ? hi[wb] : inf;
            double pa, pb, ta = 0.0, tb = 0.0, ra = 0.0, rb = 0.0;
            // one load_pair for both layouts (the per-scene one is its single-value form, where the window ends are): with a branch around
            // two forms D = 1 spills a register at the four-wave step (section 27)
            load_pair(level, level_per_pair ? e_first + e : wa, two && level_per_pair, pa, pb);
            if (!level_per_pair) pb = level[wb];
#pragma nounroll
            for (int half = 0; half < (two ? 2 : 1); ++half) {      // as k_contact: each query's searches have their own trip counts
                double t, r;
                int trips = 0;
                contact_query<D>(L, half ? qb : qa, half ? pb : pa, half ? lb : la, half ? hb : ha, 0.0, t, r, trips);
                ta = half ? ta : t; ra = half ? ra : r;
                tb = half ? t : tb; rb = half ? r : rb;
            }
            store_pair(time, e_first + e, ta, tb, two);
            if (rate) store_pair(rate, e_first + e, ra, rb, two);
        });
    });
}

// ---- the first contact of every vehicle of one fleet with every vehicle of another (rp_trajectory_cross_contact) ----
// k_versus' staging and scene arithmetic around contact_query, as k_encounter is k_fleet's: the level per scene (level_per_pair 0: n x k, read
// where the window ends are) or per pair (1: n x pairs x k, in the outputs' layout), through k_encounter's single load_pair.  Every query is
// contact_query with a delay of 0.0: k_contact's bits for the gathered pair with a null delay.
template <int D>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(D == 3 ? 2 : 4, 8)))
k_intercept(CrossSplines<D> in, size_t problems, unsigned m_a, unsigned m_b, size_t k, int P, const double *__restrict__ level, int level_per_pair,
            const double *__restrict__ lo, const double *__restrict__ hi, double *__restrict__ time, double *__restrict__ rate)
{
    __shared__ SepLds<D> L;
    const unsigned pairs = cross_pair_count(m_a, m_b);
    auto stage_problem = [&](int q, size_t p) { stage_cross_pair(L, q, in, m_a, m_b, pairs, p); };
    for_each_trip(problems, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k, s_first = p_first / pairs;
        const unsigned r_first = (unsigned)(p_first - s_first * pairs);
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            const double inf = __builtin_inf();
            const size_t sa = s_first + (r_first + (unsigned)qa) / pairs, sb = s_first + (r_first + (unsigned)qb) / pairs;
            const size_t wa = sa * k + (e - (size_t)qa * k);                            // the scene's row, the query's column
            const size_t wb = two ? sb * k + (e + 1 - (size_t)qb * k) : wa;
            const double la = lo ? lo[wa] : -inf, lb = lo ? lo[wb] : -inf, ha = hi ? hi[wa] : inf, hb = hi ? hi[wb] : inf;
            double pa, pb, ta = 0.0, tb = 0.0, ra = 0.0, rb = 0.0;
            load_pair(level, level_per_pair ? e_first + e : wa, two && level_per_pair, pa, pb);      // one form for both layouts, as k_encounter
            if (!level_per_pair) pb = level[wb];
#pragma nounroll
            for (int half = 0; half < (two ? 2 : 1); ++half) {      // as k_contact: each query's searches have their own trip counts
                double t, r;
                int trips = 0;
                contact_query<D>(L, half ? qb : qa, half ? pb : pa, half ? lb : la, half ? hb : ha, 0.0, t, r, trips);
                ta = half ? ta : t; ra = half ? ra : r;
                tb = half ? t : tb; rb = half ? r : rb;
            }
            store_pair(time, e_first + e, ta, tb, two);
            if (rate) store_pair(rate, e_first + e, ra, rb, two);
        });
    });
}

// ---- a fleet whose vehicles start at times of their own (rp_trajectory_fleet_separation_staggered, rp_trajectory_fleet_contact_staggered;
// DESIGN.md section 28) ----
// start is n x m: vehicle v of scene s runs its spline over [start, start + T] of the scene's clock, on which lo, hi and the returned time
// are.  Pair (i, j) is the pair entry's query on vehicle i's clock, each number one fp64 operation: delay = s_j - s_i, the window
// [lo - s_i, hi - s_i] (a null end is -inf / +inf before the subtraction), and the time that comes back plus s_i.  k_fleet's / k_encounter's
// staging and scene arithmetic; SepLds has no spare word and nothing may stand next to it (section 26), so the two starts of a query do
// not go through LDS: the streaming part decodes (i, j) again from the query's own problem number -- fleet_pair, at most m - 1 integer
// subtractions -- and loads the two starts as plain 8-byte loads, which L2 serves.  One query at a time does so, inside the loop over the
// pair's halves, so that one delay and one s_i are live across a query's searches and not two.  A NaN or infinite start makes the
// delay NaN or infinite (inf - inf: NaN), which is the pair entry's NaN rule for exactly that vehicle's m - 1 pairs.
struct StartOf {
    const double *__restrict__ start, *__restrict__ lo, *__restrict__ hi;
    unsigned m, pairs;

    // the query of problem r_first + q (from the trip's first scene on) at window element w: its s_i, delay and window on i's clock
    __device__ __forceinline__ void load(size_t s, unsigned r, size_t w, double &s_i, double &delay, double &l, double &h) const
    {
        const double inf = __builtin_inf();
        unsigned i, j;
        fleet_pair(r, m, i, j);
        s_i = start[s * m + i];
        delay = start[s * m + j] - s_i;
        l = (lo ? lo[w] : -inf) - s_i;
        h = (hi ? hi[w] : inf) - s_i;
    }
};

template <int D>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(D == 3 ? 2 : 4, 8)))
k_stagger(FleetSplines<D> in, size_t problems, unsigned m, size_t k, int P, const double *__restrict__ start, const double *__restrict__ lo,
          const double *__restrict__ hi, double *__restrict__ value, double *__restrict__ time, double *__restrict__ time_local)
{
    __shared__ SepLds<D> L;
    const unsigned pairs = fleet_pair_count(m);
    const StartOf clock{start, lo, hi, m, pairs};
    auto stage_problem = [&](int q, size_t p) { stage_fleet_pair(L, q, in, m, pairs, p); };
    for_each_trip(problems, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k, s_first = p_first / pairs;
        const unsigned r_first = (unsigned)(p_first - s_first * pairs);
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double va = 0.0, vb = 0.0, ta = 0.0, tb = 0.0, ua = 0.0, ub = 0.0;      // value, scene-clock time, local time
#pragma nounroll
            for (int half = 0; half < (two ? 2 : 1); ++half) {      // as k_fleet: each query's searches have their own trip counts
                const int q = half ? qb : qa;
                const unsigned r = r_first + (unsigned)q;
                const size_t s = s_first + r / pairs;
                double s_i, delay, l, h, v, t;
                clock.load(s, r % pairs, s * k + (e + (size_t)half - (size_t)q * k), s_i, delay, l, h);
                int trips = 0;
                separation_query(L, q, l, h, delay, v, t, trips);
                const double scene = t + s_i;
                va = half ? va : v; ua = half ? ua : t; ta = half ? ta : scene;
                vb = half ? v : vb; ub = half ? t : ub; tb = half ? scene : tb;
            }
            if (value) store_pair(value, e_first + e, va, vb, two);
            if (time) store_pair(time, e_first + e, ta, tb, two);
            if (time_local) store_pair(time_local, e_first + e, ua, ub, two);
        });
    });
}

template <int D>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(D == 3 ? 2 : 4, 8)))
k_rendezvous(FleetSplines<D> in, size_t problems, unsigned m, size_t k, int P, const double *__restrict__ start,
             const double *__restrict__ level, int level_per_pair, const double *__restrict__ lo, const double *__restrict__ hi,
             double *__restrict__ time, double *__restrict__ time_local, double *__restrict__ rate)
{
    __shared__ SepLds<D> L;
    const unsigned pairs = fleet_pair_count(m);
    const StartOf clock{start, lo, hi, m, pairs};
    auto stage_problem = [&](int q, size_t p) { stage_fleet_pair(L, q, in, m, pairs, p); };
    for_each_trip(problems, P, stage_problem, [&](size_t p_first, int here) {
        const size_t e_first = p_first * k, s_first = p_first / pairs;
        const unsigned r_first = (unsigned)(p_first - s_first * pairs);
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
            double ta = 0.0, tb = 0.0, ua = 0.0, ub = 0.0, ra = 0.0, rb = 0.0;      // scene-clock time, local time, rate
#pragma nounroll
            for (int half = 0; half < (two ? 2 : 1); ++half) {      // as k_encounter: each query's searches have their own trip counts
                const int q = half ? qb : qa;
                const unsigned r = r_first + (unsigned)q;
                const size_t s = s_first + r / pairs;
                const size_t w = s * k + (e + (size_t)half - (size_t)q * k);      // the scene's row, the query's column
                double s_i, delay, l, h, t, rt;
                clock.load(s, r % pairs, w, s_i, delay, l, h);
                const double p = level[level_per_pair ? e_first + e + (size_t)half : w];
                int trips = 0;
                contact_query<D>(L, q, p, l, h, delay, t, rt, trips);
                const double scene = t + s_i;
                ua = half ? ua : t; ta = half ? ta : scene; ra = half ? ra : rt;
                ub = half ? t : ub; tb = half ? scene : tb; rb = half ? rt : rb;
            }
            if (time) store_pair(time, e_first + e, ta, tb, two);
            if (time_local) store_pair(time_local, e_first + e, ua, ub, two);
            if (rate) store_pair(rate, e_first + e, ra, rb, two);
        });
    });
}

// ---- the fleet's first contacts with a broad phase in front (rp_trajectory_fleet_contact_culled, rp_trajectory_fleet_reach; DESIGN.md
// section 30) ----
// Four passes on one stream, none of which waits for another block.  k_reach: per vehicle, axis and query the least and greatest position
// over the scene's window -- stage_extrema and the position half of extrema_query, rp_trajectory_extrema's bits -- and per (vehicle, axis)
// a slack (fleet_cull.h).  k_sieve: one thread per (scene, pair); a query is far when the boxes' distance, less the slacks and the margin,
// is above its level (cull_far); a pair all of whose k queries are far is culled: its k times and rates are quiet_nan() -- what
// contact_query would have returned, section 30 has the proof -- and its keep-flag is 0.  k_shortlist_count / _scan / _scatter: the kept
// problems' indices in increasing order and their number, by a count per chunk of kShortChunk flags, one block's exclusive scan over the
// chunks' counts and a scatter in which every chunk knows where it starts: no atomics, the same list in every run.  k_shortlisted:
// k_encounter's staging and query around that list -- a trip stages up to P consecutive list entries, each through stage_fleet_pair at
// its listed problem (the list is strictly increasing, so an entry is never below its place and the decode's p - q holds), and a query
// finds its problem by loading the list entry again: SepLds has no spare word (section 26).  Its k outputs go to the problem's own place,
// one 8-byte store per query: neighbouring places are no neighbours in the output.
constexpr int kShortBlock = 256;
constexpr int kShortEach = 8;                                  // flags per thread: one 8-byte load
constexpr unsigned kShortChunk = kShortBlock * kShortEach;     // flags per chunk

template <int D> struct ReachOut { double *lo[D], *hi[D], *slack[D]; };      // per axis: n m k, n m k, n m (null: not written)
template <int D> struct SpanOut : ReachOut<D> { double *total[D], *speed[D]; };      // and n m, n m (null: not written)

template <int D>
__global__ void __launch_bounds__(kTrajBlock)
k_reach(FleetSplines<D> in, size_t vehicles, unsigned m, size_t k, int P, const double *__restrict__ lo, const double *__restrict__ hi,
        ReachOut<D> out)
{
    __shared__ ExtLds L;
#pragma unroll
    for (int x = 0; x < D; ++x) {
        double *__restrict__ const box_lo = out.lo[x], *__restrict__ const box_hi = out.hi[x], *__restrict__ const slack = out.slack[x];
        auto stage_problem = [&](int q, size_t i) {
            Knots kn = in.v[x].load(i);
            stage_extrema(L, q, kn);
            kn.check();
            if (slack) slack[i] = cull_slack(kn.p0, kn.p1, kn.p2, kn.v0, kn.v1, kn.v2, kn.t0, kn.t1);
        };
        for_each_trip(vehicles, P, stage_problem, [&](size_t p_first, int here) {
            const size_t e_first = p_first * k, s_first = p_first / m;
            const unsigned r_first = (unsigned)(p_first - s_first * m);
            stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
                const double inf = __builtin_inf();
                const size_t sa = s_first + (r_first + (unsigned)qa) / m, sb = s_first + (r_first + (unsigned)qb) / m;
                const size_t wa = sa * k + (e - (size_t)qa * k);                            // the scene's row, the query's column
                const size_t wb = two ? sb * k + (e + 1 - (size_t)qb * k) : wa;
                const double la = lo ? lo[wa] : -inf, lb = lo ? lo[wb] : -inf, ha = hi ? hi[wa] : inf, hb = hi ? hi[wb] : inf;
                Extreme Pa, Va, Pb, Vb;
                extrema_query<true, false>(L, qa, la, ha, Pa, Va);
                extrema_query<true, false>(L, qb, lb, hb, Pb, Vb);
                if (box_lo) store_pair(box_lo, e_first + e, Pa.lo_v, Pb.lo_v, two);
                if (box_hi) store_pair(box_hi, e_first + e, Pa.hi_v, Pb.hi_v, two);
            });
        });
    }
}

template <int D> struct SieveIn { const double *lo[D], *hi[D], *slack[D]; };

// a sieve thread's problem p (false: none), its scene s and its two vehicles' places
__device__ __forceinline__ bool sieve_pair(size_t problems, unsigned m, size_t &p, size_t &s, size_t &vi, size_t &vj)
{
    p = (size_t)blockIdx.x * kShortBlock + threadIdx.x;
    if (p >= problems) return false;
    const unsigned pairs = fleet_pair_count(m);
    s = p / pairs;
    unsigned i, j;
    fleet_pair((unsigned)(p - s * pairs), m, i, j);
    vi = s * m + i, vj = s * m + j;
    return true;
}

// its keep-flag, and a culled pair's NaNs in the outputs that are wanted
__device__ __forceinline__ void sieve_verdict(bool culled, size_t p, size_t k, double *__restrict__ time, double *__restrict__ time_local,
                                              double *__restrict__ rate, unsigned char *__restrict__ kept)
{
    kept[p] = culled ? 0 : 1;
    if (!culled) return;
    const double nan = quiet_nan();
    for (size_t q = 0; q < k; ++q) {
        if (time) time[p * k + q] = nan;
        if (time_local) time_local[p * k + q] = nan;
        if (rate) rate[p * k + q] = nan;
    }
}

template <int D>
__global__ void __launch_bounds__(kShortBlock)
k_sieve(SieveIn<D> box, size_t problems, unsigned m, size_t k, const double *__restrict__ level, int level_per_pair,
        double *__restrict__ time, double *__restrict__ rate, unsigned char *__restrict__ kept)
{
    size_t p, s, vi, vj;
    if (!sieve_pair(problems, m, p, s, vi, vj)) return;
    bool culled = true;
    for (size_t q = 0; q < k && culled; ++q) {
        CullBound b = cull_begin();
#pragma unroll
        for (int x = 0; x < D; ++x)
            cull_add(b, box.lo[x][vi * k + q], box.hi[x][vi * k + q], box.lo[x][vj * k + q], box.hi[x][vj * k + q], box.slack[x][vi],
                     box.slack[x][vj]);
        culled = cull_far(b, level[level_per_pair ? p * k + q : s * k + q]);
    }
    sieve_verdict(culled, p, k, time, nullptr, rate, kept);
}

// the kShortEach flags of this thread (those at or beyond `problems` count as 0), one bit each, lowest first
__device__ __forceinline__ unsigned shortlist_flags(const unsigned char *__restrict__ kept, size_t problems, size_t first)
{
    unsigned bits = 0;
    if (first + kShortEach <= problems) {      // (kept is 16-byte aligned and first a multiple of 8)
        const uint64_t w = *reinterpret_cast<const uint64_t *>(kept + first);
#pragma unroll
        for (int b = 0; b < kShortEach; ++b) bits |= ((unsigned)(w >> (8 * b)) & 0xffu) ? 1u << b : 0u;
    } else {
        for (int b = 0; b < kShortEach; ++b)
            if (first + (size_t)b < problems && kept[first + (size_t)b]) bits |= 1u << b;
    }
    return bits;
}

// the exclusive prefix sums of one value per thread over the block, and their total: kShortBlock threads, Hillis-Steele in LDS
__device__ __forceinline__ unsigned shortlist_block_scan(unsigned (&s)[kShortBlock], unsigned mine, unsigned &total)
{
    const int t = (int)threadIdx.x;
    s[t] = mine;
    __syncthreads();
    for (int step = 1; step < kShortBlock; step <<= 1) {
        const unsigned add = t >= step ? s[t - step] : 0u;
        __syncthreads();
        s[t] += add;
        __syncthreads();
    }
    total = s[kShortBlock - 1];
    const unsigned before = s[t] - mine;
    __syncthreads();
    return before;
}

__global__ void __launch_bounds__(kShortBlock)
k_shortlist_count(const unsigned char *__restrict__ kept, size_t problems, uint32_t *__restrict__ chunk_count)
{
    __shared__ unsigned s[kShortBlock];
    const size_t first = ((size_t)blockIdx.x * kShortBlock + threadIdx.x) * kShortEach;
    unsigned total;
    shortlist_block_scan(s, (unsigned)__builtin_popcount(shortlist_flags(kept, problems, first)), total);
    if (threadIdx.x == 0) chunk_count[blockIdx.x] = total;
}

// one block: chunk_count becomes where each chunk's entries start, *count their number.  Thread t takes the chunks [t each, (t + 1) each).
__global__ void __launch_bounds__(kShortBlock)
k_shortlist_scan(uint32_t *__restrict__ chunk_count, size_t chunks, uint32_t *__restrict__ count)
{
    __shared__ unsigned s[kShortBlock];
    const size_t each = (chunks + kShortBlock - 1) / kShortBlock;
    const size_t from = (size_t)threadIdx.x * each < chunks ? (size_t)threadIdx.x * each : chunks;
    const size_t to = from + each < chunks ? from + each : chunks;
    unsigned mine = 0;
    for (size_t c = from; c < to; ++c) mine += chunk_count[c];
    unsigned total;
    unsigned at = shortlist_block_scan(s, mine, total);
    for (size_t c = from; c < to; ++c) {
        const unsigned here = chunk_count[c];
        chunk_count[c] = at;
        at += here;
    }
    if (threadIdx.x == 0) *count = total;
}

__global__ void __launch_bounds__(kShortBlock)
k_shortlist_scatter(const unsigned char *__restrict__ kept, size_t problems, const uint32_t *__restrict__ chunk_start, uint32_t *__restrict__ list)
{
    __shared__ unsigned s[kShortBlock];
    const size_t first = ((size_t)blockIdx.x * kShortBlock + threadIdx.x) * kShortEach;
    const unsigned bits = shortlist_flags(kept, problems, first);
    unsigned total;
    size_t at = (size_t)chunk_start[blockIdx.x] + shortlist_block_scan(s, (unsigned)__builtin_popcount(bits), total);
    for (int b = 0; b < kShortEach; ++b)
        if (bits >> b & 1u) {
            if (at < problems) list[at] = (uint32_t)(first + (size_t)b);      // (always: there are no more kept flags than problems)
            ++at;
        }
}

// k_shortlisted (one clock) and k_appointed (STAGGERED: StartOf::load, a delay and a third output); section 32.  One clock is not a zero
// start: t + 0.0 would make a -0.0 time +0.0, so that branch has its literal 0.0 delay and stores t as it is, unasked.
template <int D, bool STAGGERED>
__device__ __forceinline__ void search_listed(FleetSplines<D> in, size_t problems, unsigned m, size_t k, int P, const double *__restrict__ start,
                                              const double *__restrict__ level, int level_per_pair, const double *__restrict__ lo,
                                              const double *__restrict__ hi, double *__restrict__ time, double *__restrict__ time_local,
                                              double *__restrict__ rate, const uint32_t *__restrict__ list, const uint32_t *__restrict__ count)
{
    __shared__ SepLds<D> L;
    const unsigned pairs = fleet_pair_count(m);
    const size_t listed = *count < problems ? (size_t)*count : problems;      // the device's own count, never beyond the list
    const size_t last = problems - 1;
    auto stage_problem = [&](int q, size_t at) {
        const size_t p = list[at];
        stage_fleet_pair(L, q, in, m, pairs, p < last ? p : last);      // (an entry is a problem: the clamp never acts)
    };
    for_each_trip(listed, P, stage_problem, [&](size_t at_first, int here) {
        stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
#pragma nounroll
            for (int half = 0; half < (two ? 2 : 1); ++half) {      // as k_encounter: each query's searches have their own trip counts
                const int q = half ? qb : qa;
                const size_t entry = list[at_first + (size_t)q], p = entry < last ? entry : last;
                const size_t col = e + (size_t)half - (size_t)q * k;
                const uint32_t s = (uint32_t)p / pairs;
                const size_t w = (size_t)s * k + col;      // the scene's row, the query's column
                const size_t o = p * k + col;              // the problem's own place
                double t, r;
                int trips = 0;
                if constexpr (STAGGERED) {
                    const StartOf clock{start, lo, hi, m, pairs};
                    double s_i, delay, l, h;
                    clock.load(s, (uint32_t)p - s * pairs, w, s_i, delay, l, h);
                    contact_query<D>(L, q, level[level_per_pair ? o : w], l, h, delay, t, r, trips);
                    if (time) time[o] = t + s_i;
                    if (time_local) time_local[o] = t;
                } else {
                    const double inf = __builtin_inf();
                    contact_query<D>(L, q, level[level_per_pair ? o : w], lo ? lo[w] : -inf, hi ? hi[w] : inf, 0.0, t, r, trips);
                    time[o] = t;
                }
                if (rate) rate[o] = r;
            }
        });
    });
}

// Budgets as k_encounter's (section 27); the hint and what the allocator does without it are in section 30.
template <int D>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(D == 3 ? 2 : 4, 8)))
k_shortlisted(FleetSplines<D> in, size_t problems, unsigned m, size_t k, int P, const double *__restrict__ level, int level_per_pair,
              const double *__restrict__ lo, const double *__restrict__ hi, double *__restrict__ time, double *__restrict__ rate,
              const uint32_t *__restrict__ list, const uint32_t *__restrict__ count)
{
    search_listed<D, false>(in, problems, m, k, P, nullptr, level, level_per_pair, lo, hi, time, nullptr, rate, list, count);
}

// ---- the broad phase with a start time per vehicle (rp_trajectory_fleet_contact_staggered_culled, rp_trajectory_fleet_reach_staggered;
// DESIGN.md section 31) ----
// The same four passes around k_rendezvous' query.  k_span: k_reach with the window of vehicle v taken on v's own clock,
// [lo - s_v, hi - s_v], StartOf::load's subtraction, so the box window of a pair's first vehicle is the search's window bit for bit; per
// (vehicle, axis) it also leaves the checked total time -- stage_vehicles' Ta / Tb -- and a bound of the spline's speed.  k_winnow: one
// thread per (scene, pair); a pair with a start that is not finite is kept; a query is out when contact_query would refuse it before its
// walk (cull_refused: its own operations on the stored totals) or when the boxes are far with the time error of t - delay allowed for
// (cull_add_staggered); a pair all of whose queries are out is culled and gets quiet_nan() in its k times, local times and rates.  The
// list kernels are section 30's.  k_appointed: k_shortlisted's staging and stores around StartOf::load and contact_query with a delay.
template <int D>
__global__ void __launch_bounds__(kTrajBlock)
k_span(FleetSplines<D> in, size_t vehicles, unsigned m, size_t k, int P, const double *__restrict__ start, const double *__restrict__ lo,
       const double *__restrict__ hi, SpanOut<D> out)
{
    __shared__ ExtLds L;
#pragma unroll
    for (int x = 0; x < D; ++x) {
        double *__restrict__ const box_lo = out.lo[x], *__restrict__ const box_hi = out.hi[x], *__restrict__ const slack = out.slack[x];
        double *__restrict__ const total = out.total[x], *__restrict__ const speed = out.speed[x];
        auto stage_problem = [&](int q, size_t i) {
            Knots kn = in.v[x].load(i);
            stage_extrema(L, q, kn);
            kn.check();
            const double T = kn.t0 + kn.t1;      // stage_vehicles' Ta / Tb
            if (slack) slack[i] = cull_slack(kn.p0, kn.p1, kn.p2, kn.v0, kn.v1, kn.v2, kn.t0, kn.t1);
            if (total) total[i] = T;
            if (speed)
                speed[i] = cull_speed(L.e.c[0][1][q], L.e.c[0][2][q], L.e.c[0][3][q], kn.t0, L.e.c[1][1][q], L.e.c[1][2][q], L.e.c[1][3][q], kn.t1, T);
        };
        for_each_trip(vehicles, P, stage_problem, [&](size_t p_first, int here) {
            const size_t e_first = p_first * k, s_first = p_first / m;
            const unsigned r_first = (unsigned)(p_first - s_first * m);
            stream_pairs(here, k, [&](size_t e, int qa, int qb, bool two) {
                const double inf = __builtin_inf();
                const size_t sa = s_first + (r_first + (unsigned)qa) / m, sb = s_first + (r_first + (unsigned)qb) / m;
                const size_t wa = sa * k + (e - (size_t)qa * k);                            // the scene's row, the query's column
                const size_t wb = two ? sb * k + (e + 1 - (size_t)qb * k) : wa;
                const double start_a = start[p_first + (size_t)qa], start_b = start[p_first + (size_t)qb];      // a problem is a vehicle
                const double la = (lo ? lo[wa] : -inf) - start_a, lb = (lo ? lo[wb] : -inf) - start_b;
                const double ha = (hi ? hi[wa] : inf) - start_a, hb = (hi ? hi[wb] : inf) - start_b;
                Extreme Pa, Va, Pb, Vb;
                extrema_query<true, false>(L, qa, la, ha, Pa, Va);
                extrema_query<true, false>(L, qb, lb, hb, Pb, Vb);
                if (box_lo) store_pair(box_lo, e_first + e, Pa.lo_v, Pb.lo_v, two);
                if (box_hi) store_pair(box_hi, e_first + e, Pa.hi_v, Pb.hi_v, two);
            });
        });
    }
}

template <int D> struct WinnowIn : SieveIn<D> { const double *total[D], *speed[D]; };

template <int D>
__global__ void __launch_bounds__(kShortBlock)
k_winnow(WinnowIn<D> box, size_t problems, unsigned m, size_t k, const double *__restrict__ start, const double *__restrict__ level,
         int level_per_pair, const double *__restrict__ lo, const double *__restrict__ hi, double *__restrict__ time,
         double *__restrict__ time_local, double *__restrict__ rate, unsigned char *__restrict__ kept)
{
    size_t p, s, vi, vj;
    if (!sieve_pair(problems, m, p, s, vi, vj)) return;
    const double inf = __builtin_inf();
    const double s_i = start[vi], s_j = start[vj];
    const double delay = s_j - s_i;      // StartOf::load's
    bool culled = cull_finite(s_i) && cull_finite(s_j);      // a start that is not finite: the search makes the NaNs
    CullDomain domain = cull_domain_begin();
#pragma unroll
    for (int x = 0; x < D; ++x) cull_domain_first(domain, box.total[x][vi]);
#pragma unroll
    for (int x = 0; x < D; ++x) cull_domain_second(domain, delay, box.total[x][vj]);
    for (size_t q = 0; q < k && culled; ++q) {
        const double l = (lo ? lo[s * k + q] : -inf) - s_i, h = (hi ? hi[s * k + q] : inf) - s_i;
        const double reach = level[level_per_pair ? p * k + q : s * k + q];
        if (cull_refused(domain, delay, reach, l, h)) continue;
        CullBound b = cull_begin();
#pragma unroll
        for (int x = 0; x < D; ++x)
            cull_add_staggered(b, box.lo[x][vi * k + q], box.hi[x][vi * k + q], box.lo[x][vj * k + q], box.hi[x][vj * k + q], box.slack[x][vi],
                               box.slack[x][vj], box.speed[x][vi], box.speed[x][vj], box.total[x][vi], box.total[x][vj]);
        culled = cull_far(b, reach);
    }
    sieve_verdict(culled, p, k, time, time_local, rate, kept);
}

// Budgets as k_rendezvous' (section 28).
template <int D>
__global__ void __launch_bounds__(kTrajBlock) __attribute__((amdgpu_waves_per_eu(D == 3 ? 2 : 4, 8)))
k_appointed(FleetSplines<D> in, size_t problems, unsigned m, size_t k, int P, const double *__restrict__ start,
            const double *__restrict__ level, int level_per_pair, const double *__restrict__ lo, const double *__restrict__ hi,
            double *__restrict__ time, double *__restrict__ time_local, double *__restrict__ rate, const uint32_t *__restrict__ list,
            const uint32_t *__restrict__ count)
{
    search_listed<D, true>(in, problems, m, k, P, start, level, level_per_pair, lo, hi, time, time_local, rate, list, count);
}

// ---- plot data ----
// Per problem 66 positions (drawSegment, onedpath_ip.cpp:1065-1088, 33 per segment) and 4 end accelerations
// (plotAcceleration, 1024-1027).  The launch moves 64 B of state in and 560 B out per problem: it has to be an HBM-write
// kernel.  A 256-thread block takes 128 problems: its first 128 threads read one problem each (through the loader) and leave,
// per segment, the six numbers a sample is made of in LDS; then all threads write the block's 8,448 positions
// and 512 accelerations as consecutive elements (full coalesced segments), each from the constants of its problem.  The
// reference's divisions are multiplications by a refined reciprocal (rcp_: IEEE 1/x), one per segment instead of nine per
// sample; the parity test allows 1e-13.  (The first form -- one thread per output element, every thread reading the eight
// fields and dividing for itself -- ran at 0.17 of the HBM peak: it was bound by its 9 broadcast loads per wave.)
// No NaN rule here (Knots::check is not called): a duration that is not positive gives what the arithmetic gives.
constexpr int kSampleProblems = 128;

template <class Load>
__device__ __forceinline__ void sample_block(const Load &from, size_t first, size_t count, double *__restrict__ pos66, double *__restrict__ acc4)
{
    __shared__ double s_seg[2][6][kSampleProblems];      // per segment: x0, x1, va, acc0, jrk0, h / 32
    __shared__ double s_acc[4][kSampleProblems];
    const size_t p_first = (size_t)blockIdx.x * kSampleProblems;      // output row of the block's first problem
    const int here = problems_here(count, p_first, kSampleProblems);
    if (threadIdx.x < here) {
        const int q = threadIdx.x;
        const Knots kn = from.load(first + p_first + q);
#pragma unroll
        for (int seg = 0; seg < 2; ++seg) {
            const double x0 = seg ? kn.p1 : kn.p0, x1 = seg ? kn.p2 : kn.p1, va = seg ? kn.v1 : kn.v0, vb = seg ? kn.v2 : kn.v1, h = seg ? kn.t1 : kn.t0;
            const double ih = rcp_<double>(h);
            double acc0, jrk0;
            segment_constants(x0, x1, va, vb, ih, acc0, jrk0);
            s_seg[seg][0][q] = x0; s_seg[seg][1][q] = x1; s_seg[seg][2][q] = va;
            s_seg[seg][3][q] = acc0; s_seg[seg][4][q] = jrk0; s_seg[seg][5][q] = h * 0.03125;
            // end accelerations of the segment (evalAccelInit / evalAccelFinal's formulas)
            s_acc[2 * seg][q] = ((x1 - x0) * 6.0 * ih + va * -4.0 + vb * -2.0) * ih;
            s_acc[2 * seg + 1][q] = ((x1 - x0) * -6.0 * ih + va * 2.0 + vb * 4.0) * ih;
        }
    }
    __syncthreads();
    // two consecutive positions per thread and trip (a problem's 66 are 33 pairs): 16-byte nontemporal stores, 1 KiB per wave
    auto position = [&](int q, int slot) -> double {
        const int seg = slot >= 33, j = slot - 33 * seg;
        if (j == 0) return s_seg[seg][0][q];
        if (j == 32) return s_seg[seg][1][q];
        const double t = s_seg[seg][5][q] * (double)j;      // h j / 32
        return cubic_pos(s_seg[seg][0][q], s_seg[seg][2][q], s_seg[seg][3][q], s_seg[seg][4][q], t);
    };
    v2 *out_pos = reinterpret_cast<v2 *>(pos66 + p_first * 66);      // 16-byte aligned: 66 doubles per problem, 128 problems per block
    for (int pr = threadIdx.x; pr < here * 33; pr += kTrajBlock) {
        const int q = pr / 33, pair = pr - q * 33;
        const v2 both = {position(q, 2 * pair), position(q, 2 * pair + 1)};
        __builtin_nontemporal_store(both, out_pos + pr);
    }
    double *out_acc = acc4 + p_first * 4;
    for (int o = threadIdx.x; o < here * 4; o += kTrajBlock) out_acc[o] = s_acc[o & 3][o >> 2];
}

// Problems [first, first + count) of a batch, rows in problem order, gathered field by field through slot_of.
// (Walking POSITIONS instead -- coalesced field reads, each problem's 528-byte row scattered to where prob_of says -- was measured
// and is slower, 0.227 against 0.194 ms at 1 Mi problems: rows start on alternating 16-byte offsets, so every row ends in two
// partial sectors.  The gather through slot_of costs eight -- with zero end velocities, which are then not read, six --
// 32-byte sectors per problem on top of the 560 B written; that traffic is what the launch time is made of.)
template <typename T, int VARIANT, bool ZV>
__global__ void __launch_bounds__(kTrajBlock)
k_sample(const T *__restrict__ base, size_t stride, size_t first, size_t count, const uint32_t *__restrict__ slot_of,
         double *__restrict__ pos66, double *__restrict__ acc4)
{
    sample_block(FromBatch<T, VARIANT, ZV>{base, stride, slot_of}, first, count, pos66, acc4);
}

// The same plot data for a WHOLE scheduled batch from two problem-order records per problem (round 4): the positions the batch
// was given (StartRecord, kept by the scheduling pass) and the problem's solution record (k_solution writes them into a scratch
// first: 68 B per problem).  Both reads are coalesced whole sectors -- 64 B per problem where the gather through slot_of touches
// six 32-byte sectors for 48 B.  Zero end velocities only, and only while the records are the batch's positions (rp_batch.cpp
// keeps the flag).
template <typename S>
__global__ void __launch_bounds__(kTrajBlock)
k_sample_records(const StartRecord *__restrict__ records, const Solution *__restrict__ sol, size_t count,
                 double *__restrict__ pos66, double *__restrict__ acc4)
{
    sample_block(FromRecords<S>{records, sol}, 0, count, pos66, acc4);
}

// problems per trip: a function of k alone; even where the pointwise kernels need a trip to start on a 16-byte boundary
int problems_per_trip(size_t k, bool even)
{
    size_t P = kTrajTrip / k;
    if (P > (size_t)kTrajProblems) P = kTrajProblems;
    if (even) P &= ~(size_t)1;
    const size_t least = even ? 2 : 1;
    return (int)(P < least ? least : P);
}

unsigned trajectory_grid(size_t n, int P)
{
    const size_t trips = (n + (size_t)P - 1) / (size_t)P;
    return (unsigned)(trips < kTrajGridCap ? trips : kTrajGridCap);
}

// lanes per problem of the reverse-mode kernels: a power of two <= 64 from k alone
int vjp_group(size_t k)
{
    const size_t units = (k & 1) == 0 ? k >> 1 : k;      // what a lane takes at a time: pairs when k is even
    int G = 1;
    while (G < 64 && (size_t)G < units) G <<= 1;
    return G;
}

// A stateless launch: the pointwise shape (P even) or, REVERSE, the reverse rules' (any P, G lanes per problem).
// launch(grid, block, P, G) enqueues the kernel.
template <bool REVERSE, class Launch> hipError_t launch_stateless(size_t n, size_t k, Launch launch)
{
    const int P = problems_per_trip(k, !REVERSE), G = REVERSE ? vjp_group(k) : 0;
    launch(dim3(trajectory_grid(n, P)), dim3(kTrajBlock), P, G);
    return hipGetLastError();
}

// A launch on a batch's current state, PROBLEM order through its slot map: one kernel per storage type, variant and zero-velocity form.
// launch(stage, grid, block, P) enqueues the kernel that the type of `stage` selects.
template <class Launch> hipError_t launch_on_batch(const BatchView &b, size_t k, Launch launch)
{
    if (b.n == 0) return hipSuccess;
    const int P = problems_per_trip(k, true);
    RP_DISPATCH(kVariant | kZeroVel, b, launch(FromBatch<S, V, Z>{(const S *)b.base, b.stride, slots(b)}, dim3(trajectory_grid(b.n, P)), dim3(kTrajBlock), P));
    return hipGetLastError();
}

// The run-time number of axes as a compile-time one: f(std::integral_constant<int, D>) for d = 1, 2, 3, a refusal for any other d.
template <class F> hipError_t with_axes(int d, F f)
{
    switch (d) {
    case 1: return f(std::integral_constant<int, 1>{});
    case 2: return f(std::integral_constant<int, 2>{});
    case 3: return f(std::integral_constant<int, 3>{});
    }
    return hipErrorInvalidValue;
}

// the kernels' tables from the entries': d_spline_a, d_spline_b and d_fleet are 8 d pointers each, axis x at 8 x
template <int D> SepSplines<D> sep_splines(const double *const *d_spline_a, const double *const *d_spline_b)
{
    SepSplines<D> in;
    for (int x = 0; x < D; ++x) {
        in.a[x] = FromArrays{table_of<8>(d_spline_a + 8 * x)};
        in.b[x] = FromArrays{table_of<8>(d_spline_b + 8 * x)};
    }
    return in;
}

template <int D> FleetSplines<D> fleet_splines(const double *const *d_fleet)
{
    FleetSplines<D> in;
    for (int x = 0; x < D; ++x) in.v[x] = FromArrays{table_of<8>(d_fleet + 8 * x)};
    return in;
}

// A pointwise launch over n pairs of vehicles in d axes: launch(axes, grid, block, P), D = decltype(axes)::value.
template <class Launch> hipError_t launch_on_pairs(size_t n, size_t k, int d, Launch launch)
{
    return with_axes(d, [&](auto axes) {
        return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) { launch(axes, grid, block, P); });
    });
}

// The same over the n m (m - 1) / 2 (scene, pair) problems of n scenes of m vehicles: launch(axes, problems, grid, block, P).
template <class Launch> hipError_t launch_on_fleet(size_t n, size_t m, size_t k, int d, Launch launch)
{
    if (m < 2 || m > kFleetMost) return hipErrorInvalidValue;
    const size_t problems = n * fleet_pair_count((unsigned)m);
    return launch_on_pairs(problems, k, d, [&](auto axes, dim3 grid, dim3 block, int P) { launch(axes, problems, grid, block, P); });
}

template <int D> CrossSplines<D> cross_splines(const double *const *d_fleet_a, const double *const *d_fleet_b)
{
    CrossSplines<D> in;
    for (int x = 0; x < D; ++x) {
        in.a[x] = FromArrays{table_of<8>(d_fleet_a + 8 * x)};
        in.b[x] = FromArrays{table_of<8>(d_fleet_b + 8 * x)};
    }
    return in;
}

// The same over the n m_a m_b (scene, pair) problems of n scenes of two fleets: launch(axes, problems, grid, block, P).
template <class Launch> hipError_t launch_on_cross(size_t n, size_t m_a, size_t m_b, size_t k, int d, Launch launch)
{
    if (m_a < 1 || m_a > kCrossMost || m_b < 1 || m_b > kCrossMost) return hipErrorInvalidValue;
    const size_t problems = n * cross_pair_count((unsigned)m_a, (unsigned)m_b);
    return launch_on_pairs(problems, k, d, [&](auto axes, dim3 grid, dim3 block, int P) { launch(axes, problems, grid, block, P); });
}

}  // namespace

hipError_t launch_trajectory_eval(size_t n, size_t k, const double *const d_spline[8], const double *d_tau, double *d_pos, double *d_vel,
                                  double *d_acc, hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_trajectory_eval, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, n, k, P, d_tau, d_pos, d_vel, d_acc);
    });
}

hipError_t launch_trajectory_jvp(size_t n, size_t k, const double *const d_spline[8], const double *d_tau, const double *const d_spline_dot[8],
                                 const double *d_tau_dot, double *d_pos_dot, double *d_vel_dot, double *d_acc_dot, hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_trajectory_jvp, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, table_of<8>(d_spline_dot), n, k, P, d_tau,
                           d_tau_dot, d_pos_dot, d_vel_dot, d_acc_dot);
    });
}

hipError_t launch_trajectory_vjp(size_t n, size_t k, const double *const d_spline[8], const double *d_tau, const double *d_g_pos,
                                 const double *d_g_vel, const double *d_g_acc, double *const d_spline_bar[8], double *d_tau_bar, hipStream_t stream)
{
    return launch_stateless<true>(n, k, [&](dim3 grid, dim3 block, int P, int G) {
        hipLaunchKernelGGL(k_trajectory_vjp, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, n, k, P, G, d_tau, d_g_pos, d_g_vel, d_g_acc,
                           table_of<8>(d_spline_bar), d_tau_bar);
    });
}

hipError_t launch_trajectory_hvp(size_t n, size_t k, const double *const d_spline[8], const double *d_tau, const double *d_g_pos,
                                 const double *d_g_vel, const double *d_g_acc, const double *const d_spline_dot[8], const double *d_tau_dot,
                                 double *const d_spline_bar_dot[8], double *d_tau_bar_dot, hipStream_t stream)
{
    return launch_stateless<true>(n, k, [&](dim3 grid, dim3 block, int P, int G) {
        hipLaunchKernelGGL(k_trajectory_hvp, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, table_of<8>(d_spline_dot), n, k, P, G, d_tau,
                           d_g_pos, d_g_vel, d_g_acc, d_tau_dot, table_of<8>(d_spline_bar_dot), d_tau_bar_dot);
    });
}

hipError_t launch_trajectory_batch(const BatchView &b, const double *d_tau, size_t k, double *d_pos, double *d_vel, double *d_acc, hipStream_t stream)
{
    return launch_on_batch(b, k, [&](auto stage, dim3 grid, dim3 block, int P) {
        hipLaunchKernelGGL(k_batch_trajectory, grid, block, 0, stream, stage, b.n, k, P, d_tau, d_pos, d_vel, d_acc);
    });
}

hipError_t launch_crossing(size_t n, size_t k, const double *const d_spline[8], const double *d_level, double *d_time, double *d_vel, hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_crossing, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, n, k, P, d_level, d_time, d_vel);
    });
}

hipError_t launch_crossing_batch(const BatchView &b, const double *d_level, size_t k, double *d_time, double *d_vel, hipStream_t stream)
{
    return launch_on_batch(b, k, [&](auto stage, dim3 grid, dim3 block, int P) {
        hipLaunchKernelGGL(k_batch_crossing, grid, block, 0, stream, stage, b.n, k, P, d_level, d_time, d_vel);
    });
}

hipError_t launch_extrema(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi, double *const d_value[4],
                          double *const d_time[4], hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_extrema, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, n, k, P, d_lo, d_hi, table_of<4>(d_value),
                           table_of<4>(d_time));
    });
}

hipError_t launch_extrema_batch(const BatchView &b, const double *d_lo, const double *d_hi, size_t k, double *const d_value[4],
                                double *const d_time[4], hipStream_t stream)
{
    return launch_on_batch(b, k, [&](auto stage, dim3 grid, dim3 block, int P) {
        hipLaunchKernelGGL(k_batch_extrema, grid, block, 0, stream, stage, b.n, k, P, d_lo, d_hi, table_of<4>(d_value), table_of<4>(d_time));
    });
}

hipError_t launch_integrals(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi, double *const d_value[4],
                            hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_integrals, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, n, k, P, d_lo, d_hi, table_of<4>(d_value));
    });
}

hipError_t launch_integrals_batch(const BatchView &b, const double *d_lo, const double *d_hi, size_t k, double *const d_value[4], hipStream_t stream)
{
    return launch_on_batch(b, k, [&](auto stage, dim3 grid, dim3 block, int P) {
        hipLaunchKernelGGL(k_batch_integrals, grid, block, 0, stream, stage, b.n, k, P, d_lo, d_hi, table_of<4>(d_value));
    });
}

hipError_t launch_integrals_jvp(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi,
                                const double *const d_spline_dot[8], const double *d_lo_dot, const double *d_hi_dot, double *const d_value_dot[4],
                                hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_jvp_integrals, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, table_of<8>(d_spline_dot), n, k, P, d_lo, d_hi,
                           d_lo_dot, d_hi_dot, table_of<4>(d_value_dot));
    });
}

hipError_t launch_integrals_vjp(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi, const double *const d_g[4],
                                double *const d_spline_bar[8], double *d_lo_bar, double *d_hi_bar, hipStream_t stream)
{
    return launch_stateless<true>(n, k, [&](dim3 grid, dim3 block, int P, int G) {
        hipLaunchKernelGGL(k_vjp_integrals, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, n, k, P, G, d_lo, d_hi, table_of<4>(d_g),
                           table_of<8>(d_spline_bar), d_lo_bar, d_hi_bar);
    });
}

hipError_t launch_integrals_hvp(size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi, const double *const d_g[4],
                                const double *const d_spline_dot[8], const double *d_lo_dot, const double *d_hi_dot,
                                double *const d_spline_bar_dot[8], double *d_lo_bar_dot, double *d_hi_bar_dot, hipStream_t stream)
{
    return launch_stateless<true>(n, k, [&](dim3 grid, dim3 block, int P, int G) {
        hipLaunchKernelGGL(k_window_hvp, grid, block, 0, stream, FromArrays{table_of<8>(d_spline)}, table_of<8>(d_spline_dot), n, k, P, G, d_lo, d_hi,
                           table_of<4>(d_g), d_lo_dot, d_hi_dot, table_of<8>(d_spline_bar_dot), d_lo_bar_dot, d_hi_bar_dot);
    });
}

hipError_t launch_gap(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                      const double *d_hi, const double *d_delay, double *const d_value[2], double *const d_time[2], hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_gap, grid, block, 0, stream, FromArrays{table_of<8>(d_spline_a)}, FromArrays{table_of<8>(d_spline_b)}, n, k, P, d_lo,
                           d_hi, d_delay, table_of<2>(d_value), table_of<2>(d_time));
    });
}

hipError_t launch_tracking(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                           const double *d_hi, const double *d_delay, double *const d_value[3], hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_tracking, grid, block, 0, stream, FromArrays{table_of<8>(d_spline_a)}, FromArrays{table_of<8>(d_spline_b)}, n, k, P,
                           d_lo, d_hi, d_delay, table_of<3>(d_value));
    });
}

hipError_t launch_tracking_jvp(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                               const double *d_hi, const double *d_delay, const double *const d_spline_a_dot[8],
                               const double *const d_spline_b_dot[8], const double *d_lo_dot, const double *d_hi_dot, const double *d_delay_dot,
                               double *const d_value_dot[3], hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_tracking_jvp, grid, block, 0, stream, FromArrays{table_of<8>(d_spline_a)}, FromArrays{table_of<8>(d_spline_b)},
                           table_of<8>(d_spline_a_dot), table_of<8>(d_spline_b_dot), n, k, P, d_lo, d_hi, d_delay, d_lo_dot, d_hi_dot, d_delay_dot,
                           table_of<3>(d_value_dot));
    });
}

// one launch per spline, back to back on the stream: side A's (made if any of its eight gradients or of lo_bar, hi_bar, delay_bar is
// wanted) writes the three per-query gradients, side B's is made if any of its eight is wanted
hipError_t launch_tracking_vjp(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                               const double *d_hi, const double *d_delay, const double *const d_g[3], double *const d_spline_a_bar[8],
                               double *const d_spline_b_bar[8], double *d_lo_bar, double *d_hi_bar, double *d_delay_bar, hipStream_t stream)
{
    bool side_a = d_lo_bar || d_hi_bar || d_delay_bar, side_b = false;
    for (int f = 0; f < 8; ++f) {
        side_a = side_a || d_spline_a_bar[f];
        side_b = side_b || d_spline_b_bar[f];
    }
    hipError_t e = hipSuccess;
    if (side_a)
        e = launch_stateless<true>(n, k, [&](dim3 grid, dim3 block, int P, int G) {
            hipLaunchKernelGGL(k_tracking_vjp<0>, grid, block, 0, stream, FromArrays{table_of<8>(d_spline_a)}, FromArrays{table_of<8>(d_spline_b)}, n,
                               k, P, G, d_lo, d_hi, d_delay, table_of<3>(d_g), table_of<8>(d_spline_a_bar), d_lo_bar, d_hi_bar, d_delay_bar);
        });
    if (e == hipSuccess && side_b)
        e = launch_stateless<true>(n, k, [&](dim3 grid, dim3 block, int P, int G) {
            hipLaunchKernelGGL(k_tracking_vjp<1>, grid, block, 0, stream, FromArrays{table_of<8>(d_spline_a)}, FromArrays{table_of<8>(d_spline_b)}, n,
                               k, P, G, d_lo, d_hi, d_delay, table_of<3>(d_g), table_of<8>(d_spline_b_bar), (double *)nullptr, (double *)nullptr,
                               (double *)nullptr);
        });
    return e;
}

// the same two launches for the reverse rule's derivative along a direction
hipError_t launch_tracking_hvp(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_lo,
                               const double *d_hi, const double *d_delay, const double *const d_g[3], const double *const d_spline_a_dot[8],
                               const double *const d_spline_b_dot[8], const double *d_lo_dot, const double *d_hi_dot, const double *d_delay_dot,
                               double *const d_spline_a_bar_dot[8], double *const d_spline_b_bar_dot[8], double *d_lo_bar_dot,
                               double *d_hi_bar_dot, double *d_delay_bar_dot, hipStream_t stream)
{
    bool side_a = d_lo_bar_dot || d_hi_bar_dot || d_delay_bar_dot, side_b = false;
    for (int f = 0; f < 8; ++f) {
        side_a = side_a || d_spline_a_bar_dot[f];
        side_b = side_b || d_spline_b_bar_dot[f];
    }
    hipError_t e = hipSuccess;
    if (side_a)
        e = launch_stateless<true>(n, k, [&](dim3 grid, dim3 block, int P, int G) {
            hipLaunchKernelGGL(k_pair_hvp<0>, grid, block, 0, stream, table_of<8>(d_spline_a), table_of<8>(d_spline_b), table_of<8>(d_spline_a_dot),
                               table_of<8>(d_spline_b_dot), n, k, P, G, d_lo, d_hi, d_delay, table_of<3>(d_g), d_lo_dot, d_hi_dot, d_delay_dot,
                               table_of<8>(d_spline_a_bar_dot), d_lo_bar_dot, d_hi_bar_dot, d_delay_bar_dot);
        });
    if (e == hipSuccess && side_b)
        e = launch_stateless<true>(n, k, [&](dim3 grid, dim3 block, int P, int G) {
            hipLaunchKernelGGL(k_pair_hvp<1>, grid, block, 0, stream, table_of<8>(d_spline_a), table_of<8>(d_spline_b), table_of<8>(d_spline_a_dot),
                               table_of<8>(d_spline_b_dot), n, k, P, G, d_lo, d_hi, d_delay, table_of<3>(d_g), d_lo_dot, d_hi_dot, d_delay_dot,
                               table_of<8>(d_spline_b_bar_dot), (double *)nullptr, (double *)nullptr, (double *)nullptr);
        });
    return e;
}

hipError_t launch_meeting(size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8], const double *d_level,
                          const double *d_lo, const double *d_hi, const double *d_delay, double *d_time, double *d_relvel, hipStream_t stream)
{
    return launch_stateless<false>(n, k, [&](dim3 grid, dim3 block, int P, int) {
        hipLaunchKernelGGL(k_meeting, grid, block, 0, stream, FromArrays{table_of<8>(d_spline_a)}, FromArrays{table_of<8>(d_spline_b)}, n, k, P,
                           d_level, d_lo, d_hi, d_delay, d_time, d_relvel);
    });
}

hipError_t launch_separation(size_t n, size_t k, int d, const double *const *d_spline_a, const double *const *d_spline_b, const double *d_lo,
                             const double *d_hi, const double *d_delay, double *d_value, double *d_time, hipStream_t stream)
{
    return launch_on_pairs(n, k, d, [&](auto axes, dim3 grid, dim3 block, int P) {
        constexpr int D = decltype(axes)::value;
        hipLaunchKernelGGL(k_separation<D>, grid, block, 0, stream, sep_splines<D>(d_spline_a, d_spline_b), n, k, P, d_lo, d_hi, d_delay, d_value,
                           d_time);
    });
}

hipError_t launch_contact(size_t n, size_t k, int d, const double *const *d_spline_a, const double *const *d_spline_b, const double *d_level_sq,
                          const double *d_lo, const double *d_hi, const double *d_delay, double *d_time, double *d_rate, hipStream_t stream)
{
    return launch_on_pairs(n, k, d, [&](auto axes, dim3 grid, dim3 block, int P) {
        constexpr int D = decltype(axes)::value;
        hipLaunchKernelGGL(k_contact<D>, grid, block, 0, stream, sep_splines<D>(d_spline_a, d_spline_b), n, k, P, d_level_sq, d_lo, d_hi, d_delay,
                           d_time, d_rate);
    });
}

hipError_t launch_fleet_separation(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_lo, const double *d_hi,
                                   double *d_value, double *d_time, hipStream_t stream)
{
    return launch_on_fleet(n, m, k, d, [&](auto axes, size_t problems, dim3 grid, dim3 block, int P) {
        constexpr int D = decltype(axes)::value;
        hipLaunchKernelGGL(k_fleet<D>, grid, block, 0, stream, fleet_splines<D>(d_fleet), problems, (unsigned)m, k, P, d_lo, d_hi, d_value, d_time);
    });
}

hipError_t launch_fleet_contact(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_level_sq, int level_per_pair,
                                const double *d_lo, const double *d_hi, double *d_time, double *d_rate, hipStream_t stream)
{
    if (!d_level_sq || !d_time) return hipErrorInvalidValue;
    return launch_on_fleet(n, m, k, d, [&](auto axes, size_t problems, dim3 grid, dim3 block, int P) {
        constexpr int D = decltype(axes)::value;
        hipLaunchKernelGGL(k_encounter<D>, grid, block, 0, stream, fleet_splines<D>(d_fleet), problems, (unsigned)m, k, P, d_level_sq,
                           level_per_pair, d_lo, d_hi, d_time, d_rate);
    });
}

hipError_t launch_cross_separation(size_t n, size_t m_a, size_t m_b, size_t k, int d, const double *const *d_fleet_a, const double *const *d_fleet_b,
                                   const double *d_lo, const double *d_hi, double *d_value, double *d_time, hipStream_t stream)
{
    return launch_on_cross(n, m_a, m_b, k, d, [&](auto axes, size_t problems, dim3 grid, dim3 block, int P) {
        constexpr int D = decltype(axes)::value;
        hipLaunchKernelGGL(k_versus<D>, grid, block, 0, stream, cross_splines<D>(d_fleet_a, d_fleet_b), problems, (unsigned)m_a, (unsigned)m_b, k, P,
                           d_lo, d_hi, d_value, d_time);
    });
}

hipError_t launch_cross_contact(size_t n, size_t m_a, size_t m_b, size_t k, int d, const double *const *d_fleet_a, const double *const *d_fleet_b,
                                const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi, double *d_time,
                                double *d_rate, hipStream_t stream)
{
    if (!d_level_sq || !d_time) return hipErrorInvalidValue;
    return launch_on_cross(n, m_a, m_b, k, d, [&](auto axes, size_t problems, dim3 grid, dim3 block, int P) {
        constexpr int D = decltype(axes)::value;
        hipLaunchKernelGGL(k_intercept<D>, grid, block, 0, stream, cross_splines<D>(d_fleet_a, d_fleet_b), problems, (unsigned)m_a, (unsigned)m_b, k,
                           P, d_level_sq, level_per_pair, d_lo, d_hi, d_time, d_rate);
    });
}

hipError_t launch_fleet_separation_staggered(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_start,
                                             const double *d_lo, const double *d_hi, double *d_value, double *d_time, double *d_time_local,
                                             hipStream_t stream)
{
    if (!d_start) return hipErrorInvalidValue;
    return launch_on_fleet(n, m, k, d, [&](auto axes, size_t problems, dim3 grid, dim3 block, int P) {
        constexpr int D = decltype(axes)::value;
        hipLaunchKernelGGL(k_stagger<D>, grid, block, 0, stream, fleet_splines<D>(d_fleet), problems, (unsigned)m, k, P, d_start, d_lo, d_hi,
                           d_value, d_time, d_time_local);
    });
}

hipError_t launch_fleet_contact_staggered(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_start,
                                          const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi, double *d_time,
                                          double *d_time_local, double *d_rate, hipStream_t stream)
{
    if (!d_start || !d_level_sq) return hipErrorInvalidValue;
    return launch_on_fleet(n, m, k, d, [&](auto axes, size_t problems, dim3 grid, dim3 block, int P) {
        constexpr int D = decltype(axes)::value;
        hipLaunchKernelGGL(k_rendezvous<D>, grid, block, 0, stream, fleet_splines<D>(d_fleet), problems, (unsigned)m, k, P, d_start, d_level_sq,
                           level_per_pair, d_lo, d_hi, d_time, d_time_local, d_rate);
    });
}

// the boxes of either clock: d_start null, k_reach (which has no totals and no speed bounds: d_total and d_speed are not looked at); given, k_span
hipError_t launch_fleet_reach(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_start, const double *d_lo,
                              const double *d_hi, double *const *d_min, double *const *d_max, double *const *d_slack, double *const *d_total,
                              double *const *d_speed, hipStream_t stream)
{
    if (m < 2 || m > kFleetMost) return hipErrorInvalidValue;
    return launch_on_pairs(n * m, k, d, [&](auto axes, dim3 grid, dim3 block, int P) {
        constexpr int D = decltype(axes)::value;
        SpanOut<D> out;
        for (int x = 0; x < D; ++x) {
            out.lo[x] = d_min ? d_min[x] : nullptr;
            out.hi[x] = d_max ? d_max[x] : nullptr;
            out.slack[x] = d_slack ? d_slack[x] : nullptr;
            out.total[x] = d_total ? d_total[x] : nullptr;
            out.speed[x] = d_speed ? d_speed[x] : nullptr;
        }
        if (d_start)
            hipLaunchKernelGGL(k_span<D>, grid, block, 0, stream, fleet_splines<D>(d_fleet), n * m, (unsigned)m, k, P, d_start, d_lo, d_hi, out);
        else
            hipLaunchKernelGGL(k_reach<D>, grid, block, 0, stream, fleet_splines<D>(d_fleet), n * m, (unsigned)m, k, P, d_lo, d_hi,
                               ReachOut<D>(out));
    });
}

namespace {

// The n m arrays the broad phase keeps per axis: the slacks; with a start per vehicle (section 31) the totals and the speed bounds too.
constexpr int cull_per_vehicle(bool staggered) { return staggered ? 3 : 1; }

// The culled entries' workspace, every part on a 16-byte boundary: per axis the boxes' two n m k arrays; per axis the n m slacks and,
// staggered, totals and speed bounds (null otherwise); the n x pairs keep-flags, the list, the chunks' counts, the count.
struct CullWorkspace {
    double *box_lo[3], *box_hi[3], *slack[3], *total[3], *speed[3];      // (axes at or beyond d: null)
    unsigned char *kept;
    uint32_t *list, *chunk, *count;
    size_t problems, chunks, bytes;
};

size_t round16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }

// the parts of a workspace at d_workspace; a null d_workspace gives the sizes, and pointers that are only offsets
CullWorkspace cull_workspace(size_t n, size_t m, size_t k, int d, bool staggered, void *d_workspace)
{
    CullWorkspace w{};
    w.problems = n * fleet_pair_count((unsigned)m);
    w.chunks = (w.problems + kShortChunk - 1) / kShortChunk;
    const size_t box_each = round16(n * m * k * sizeof(double)), slack_each = round16(n * m * sizeof(double));
    double **const per_vehicle[3] = {w.slack, w.total, w.speed};
    uintptr_t at = (uintptr_t)d_workspace;
    auto take = [&](size_t bytes) { void *const here = (void *)at; at += bytes; return here; };
    for (int x = 0; x < d; ++x) {
        w.box_lo[x] = (double *)take(box_each);
        w.box_hi[x] = (double *)take(box_each);
    }
    for (int x = 0; x < d; ++x)
        for (int a = 0; a < cull_per_vehicle(staggered); ++a) per_vehicle[a][x] = (double *)take(slack_each);
    w.kept = (unsigned char *)take(round16(w.problems));
    w.list = (uint32_t *)take(round16(w.problems * sizeof(uint32_t)));
    w.chunk = (uint32_t *)take(round16(w.chunks * sizeof(uint32_t)));
    w.count = (uint32_t *)take(16);
    w.bytes = (size_t)(at - (uintptr_t)d_workspace);
    return w;
}

// the list of the kept problems and its length from the flags (section 30's third pass)
hipError_t launch_shortlist(const CullWorkspace &w, hipStream_t stream)
{
    hipLaunchKernelGGL(k_shortlist_count, dim3((unsigned)w.chunks), dim3(kShortBlock), 0, stream, w.kept, w.problems, w.chunk);
    hipLaunchKernelGGL(k_shortlist_scan, dim3(1), dim3(kShortBlock), 0, stream, w.chunk, w.chunks, w.count);
    hipLaunchKernelGGL(k_shortlist_scatter, dim3((unsigned)w.chunks), dim3(kShortBlock), 0, stream, w.kept, w.problems, w.chunk, w.list);
    return hipGetLastError();
}

}  // namespace

size_t fleet_cull_workspace_bytes(size_t n, size_t m, size_t k, int d, bool staggered)
{
    if (m < 2 || m > kFleetMost || d < 1 || d > 3 || n == 0 || k == 0) return 0;
    if (n > (((size_t)1 << 32) - 1) / fleet_pair_count((unsigned)m)) return 0;      // a list entry is 32 bits
    if (k > SIZE_MAX / 64 / (n * m)) return 0;                                       // the boxes' bytes fit
    return cull_workspace(n, m, k, d, staggered, nullptr).bytes;
}

// The four passes of sections 30 and 31.  d_start null: one clock, k_sieve and k_shortlisted, and d_time_local is not looked at.
hipError_t launch_fleet_contact_culled(size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_start,
                                       const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi, double *d_time,
                                       double *d_time_local, double *d_rate, void *d_workspace, unsigned char *d_kept, uint32_t *d_list,
                                       uint32_t *d_count, hipStream_t stream)
{
    const bool staggered = d_start != nullptr;
    if (!d_level_sq || !d_workspace || fleet_cull_workspace_bytes(n, m, k, d, staggered) == 0) return hipErrorInvalidValue;
    const CullWorkspace w = cull_workspace(n, m, k, d, staggered, d_workspace);
    hipError_t e = launch_fleet_reach(n, m, k, d, d_fleet, d_start, d_lo, d_hi, w.box_lo, w.box_hi, w.slack, w.total, w.speed, stream);
    if (e != hipSuccess) return e;
    e = with_axes(d, [&](auto axes) {
        constexpr int D = decltype(axes)::value;
        const dim3 grid((unsigned)((w.problems + kShortBlock - 1) / kShortBlock)), block(kShortBlock);
        WinnowIn<D> box;
        for (int x = 0; x < D; ++x) { box.lo[x] = w.box_lo[x]; box.hi[x] = w.box_hi[x]; box.slack[x] = w.slack[x]; box.total[x] = w.total[x]; box.speed[x] = w.speed[x]; }
        if (staggered)
            hipLaunchKernelGGL(k_winnow<D>, grid, block, 0, stream, box, w.problems, (unsigned)m, k, d_start, d_level_sq, level_per_pair, d_lo, d_hi,
                               d_time, d_time_local, d_rate, w.kept);
        else
            hipLaunchKernelGGL(k_sieve<D>, grid, block, 0, stream, SieveIn<D>(box), w.problems, (unsigned)m, k, d_level_sq, level_per_pair, d_time,
                               d_rate, w.kept);
        return hipGetLastError();
    });
    if (e != hipSuccess) return e;
    e = launch_shortlist(w, stream);
    if (e != hipSuccess) return e;
    if (staggered ? d_time || d_time_local || d_rate : d_time != nullptr) {      // (k_shortlisted stores its time unasked)
        e = launch_on_fleet(n, m, k, d, [&](auto axes, size_t problems, dim3 grid, dim3 block, int P) {
            constexpr int D = decltype(axes)::value;
            if (staggered)
                hipLaunchKernelGGL(k_appointed<D>, grid, block, 0, stream, fleet_splines<D>(d_fleet), problems, (unsigned)m, k, P, d_start,
                                   d_level_sq, level_per_pair, d_lo, d_hi, d_time, d_time_local, d_rate, w.list, w.count);
            else
                hipLaunchKernelGGL(k_shortlisted<D>, grid, block, 0, stream, fleet_splines<D>(d_fleet), problems, (unsigned)m, k, P, d_level_sq,
                                   level_per_pair, d_lo, d_hi, d_time, d_rate, w.list, w.count);
        });
        if (e != hipSuccess) return e;
    }
    if (d_kept) e = hipMemcpyAsync(d_kept, w.kept, w.problems, hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess && d_list) e = hipMemcpyAsync(d_list, w.list, w.problems * sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
    if (e == hipSuccess && d_count) e = hipMemcpyAsync(d_count, w.count, sizeof(uint32_t), hipMemcpyDeviceToDevice, stream);
    return e;
}

// ---- plot data by problem index: a range [first, first + count) of problems, wherever they lie in the batch ----
hipError_t launch_sample_range(const BatchView &b, size_t first, size_t count, double *d_pos66, double *d_acc4, hipStream_t stream)
{
    if (count == 0) return hipSuccess;
    const dim3 grid((unsigned)((count + kSampleProblems - 1) / kSampleProblems));
    RP_DISPATCH(kVariant | kZeroVel, b, hipLaunchKernelGGL((k_sample<S, V, Z>), grid, dim3(kTrajBlock), 0, stream,
                                                           (const S *)b.base, b.stride, first, count, slots(b), d_pos66, d_acc4));
    return hipGetLastError();
}

hipError_t launch_sample(const BatchView &b, double *d_pos66, double *d_acc4, hipStream_t stream) { return launch_sample_range(b, 0, b.n, d_pos66, d_acc4, stream); }

hipError_t launch_sample_from_records(const BatchView &b, Solution *d_solution_scratch, double *d_pos66, double *d_acc4, hipStream_t stream)
{
    if (b.n == 0) return hipSuccess;
    if (!b.scheduled || !b.zero_end_vel || !b.records) return hipErrorInvalidValue;
    hipError_t e = launch_solution(b, d_solution_scratch, stream);      // every problem's (vel1, duration0, duration1) in problem order
    if (e != hipSuccess) return e;
    const dim3 grid((unsigned)((b.n + kSampleProblems - 1) / kSampleProblems));
    RP_DISPATCH(kStorage, b, hipLaunchKernelGGL((k_sample_records<S>), grid, dim3(kTrajBlock), 0, stream,
                                                (const StartRecord *)b.records, (const Solution *)d_solution_scratch, b.n, d_pos66, d_acc4));
    return hipGetLastError();
}

}  // namespace rp
