// rp_batch.cpp -- implementation of the C ABI in include/rp_batch.h over the HIP kernels.
//
// Owns, per batch: the SoA state in HBM (one allocation, `fields` arrays of `stride`
// elements), the per-problem progress words, a small scratch for reductions and the
// AoS staging buffer used by set_state/get_state.  No CPU fallback exists: without a HIP
// device every entry point that needs one fails with RP_ERR_NO_DEVICE.
#include "../../include/rp_batch.h"

#include <hip/hip_runtime_api.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstdint>
#include <cstring>
#include <atomic>
#include <initializer_list>
#include <mutex>
#include <new>

#include "ip_kernels.h"

// ---- what a batch remembers about its own state, and the only events that change it ----
// The flags below decide what a gated solve does next (start formed in registers / plain / watching for fixed points / in rounds), whether a
// bound solution buffer is seeded first and whether the plot data may go through the records.  They are assigned by the transition functions
// under the struct and nowhere else: an entry point says what happened by calling one; the questions have one predicate each, below those.
//   view.scheduled     the problems lie in the scheduled order (slot_of / prob_of), not in problem order
//   view.zero_end_vel  every end velocity is zero: the Newton kernels' zero-velocity instantiations
//   at_start           lazy: the batch holds its order and records, the feasible start itself (mutable fields, progress words) is not written:
//                      the fused solve forms it in registers, everything else goes through materialize() first (left_lazy_start, both)
//   records_current    view.records hold the positions the batch's constant fields hold
//   vel_start          the problems were given with end velocities: a restart keeps them
//   unpredicted        the order no longer predicts step counts: the fused solve runs the kernel that watches for fixed points, in ONE
//                      launch (rp_params.handoff_rounds = 0; rounds only on request, 2..8; -1: the plain kernel always)
//   sol_stale          a bound buffer's records of problems the next gated launch does NOT work on are not current: it is seeded first
//   raw_state_out      a raw pointer to a MUTABLE field is out and the caller may write at any later time: a bound buffer is seeded before EVERY
//                      gated launch that may skip problems, until the batch is given a new state (not a restart)
//   raw_positions_out  a raw pointer to a CONSTANT field (a position, an end velocity) is out: the records may miss positions written at any
//                      later time.  Never cleared: the records path of the plot data stays off for the life of the batch
//   ungated_steps      ungated steps per problem since the last init; with the device's progress words "the progress"
// event (transition): entry points -> what it leaves
//   created: create -> the zeroed struct: not scheduled, zero_end_vel, everything else false
//   identical_problems: init_default, init_stuck -> not scheduled, zero_end_vel, predicted, not lazy, records not current, no raw state out,
//       no velocity start, stale; progress reset
//   problems_given: set_problems(_device), rp_pipeline_submit -> scheduled, zero_end_vel (the velocity fields cleared first if they might be
//       non-zero), predicted, LAZY, records current, no raw state out, no velocity start, stale, no ungated steps
//   problems_vel_given: set_problems_vel(_device) -> scheduled, NOT zero_end_vel, unpredicted, start written out, records not current, no raw
//       state out, velocity start, stale, no ungated steps
//   rows_given: set_state -> scheduled by the rows' positions, zero_end_vel as scanned on the host, unpredicted, not lazy, records not current,
//       no raw state out, no velocity start, stale; progress reset
//   restarted: restart -> stale; predicted again unless a raw position pointer is out; a lazy batch is only written out and resets nothing,
//       any other goes back to its velocity start (unpredicted) or its rest-to-rest start (zero_end_vel), progress reset; raw_state_out stays
//   stepped / moved / nudged: step, step_counted / move_toward_feasibility / nudge -> stale; steps add to ungated_steps; a move or a nudge:
//       unpredicted; a nudged constant: records not current; an end velocity nudged by a non-zero delta: not zero_end_vel
//   raw_pointer_out: field_ptr (start written out first) -> records not current, stale, unpredicted, raw_positions_out or raw_state_out,
//       an end-velocity field: not zero_end_vel
//   solution_bound: bind_solution -> stale.     solution_current: solve, solve_launch -> not stale, only behind a launch that succeeded
struct rp_overlap;      // the lanes of a caller stream: below, "overlap of back-to-back fused solves"

struct rp_batch {
    rp::BatchView view;
    rp::HostParams params;
    int device;
    hipStream_t stream;
    bool own_stream;
    double *d_scratch;        // [0..4095] block partials, [4096..4099] reduction result
    double *d_aos;            // lazily allocated n * state_len doubles
    double *d_pos;            // lazily allocated 3 * n doubles (set_problems staging)
    double *d_range;          // lazily allocated kRangeChunk * kRangeRow doubles: staging of the *_range read-backs
    uint32_t *d_words;        // lazily allocated 2 n words: per-problem words gathered from batch order into problem order
    void *d_sched;            // lazily allocated scratch of the scheduling pass (schedule.hip), sched_bytes bytes
    size_t sched_bytes;
    rp::Solution *d_solscratch;   // lazily allocated n solution records: the plot data of a whole batch reads its state through them
    bool slim_schedule;       // configuration: the scheduling pass runs in its one-wave-per-block form (schedule.hip): set by rp_pipeline for its batches
    bool at_start, records_current, vel_start, unpredicted, sol_stale, raw_state_out, raw_positions_out;      // see above
    double ungated_steps;
    unsigned long long *h_pinned;   // 72 pinned host words: [0,64) counter shards, [64,68) reduction: read-backs without pageable staging
    hipEvent_t events[8];
    bool event_live[8];
    rp_overlap *lanes;        // the overlap context of `stream` (one per device and stream, shared by every batch on it); holds a reference
    uint64_t s_ticket;        // ticket of the last operation of this batch enqueued on the caller's stream
    uint64_t aux_seq;         // number of its last solve on the auxiliary lane (0: none)
    bool pipelined;           // configuration: a slot of an rp_pipeline (its stream is swapped for the scheduling pass): never overlapped
};

namespace {

thread_local char g_err[512] = "";

int fail(int status, const char *fmt, ...)
{
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof g_err, fmt, ap);
    va_end(ap);
    return status;
}

#define RP_HIP(call)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (call);                                                             \
        if (e_ != hipSuccess)                                                               \
            return fail(e_ == hipErrorOutOfMemory ? RP_ERR_NOMEM : RP_ERR_DEVICE, "%s: %s", #call, hipGetErrorString(e_)); \
    } while (0)

// ---- overlap of back-to-back fused solves of batches that share a stream ----
// A launch's wave slots empty out while its last chunks drain, and the next launch on the same stream starts only once the previous one
// has retired.  A fused solve of a materialised batch touches nothing but memory the library owns, so consecutive solves of DIFFERENT
// batches on one caller stream S may run side by side: every second one goes to an auxiliary stream ("aux") that the library keeps beside
// S.  One context per (device, S), shared by every batch created on S; each batch holds a reference from create to destroy, the last
// reference destroys aux, the events and -- where a batch created S -- S itself, so the batch that owns S may go before its borrowers.
//
// The ordering rule (the whole correctness argument).  Every operation the library enqueues takes a ticket from the context.
//   * Eligible solves (rp_batch_solve: the list there) alternate between S and aux as long as they follow one another directly; one
//     that follows anything else runs on S.
//   * `fork` is an event recorded on S.  It is (re)recorded only if the library has enqueued something on S since it was recorded last
//     (dirty_ticket > fork_ticket); eligible solves on S do not count for other batches.  It is recorded ahead of an S-lane solve
//     already (choose_lane says when), so that the aux solve that follows waits for what preceded that solve and not for the solve.
//   * An aux launch of batch b needs b's last S-side operation at or before the recorded fork (b->s_ticket <= fork_ticket): if not,
//     fork is re-recorded first.  aux waits on fork whenever it has been re-recorded; aux is in order, so an earlier aux solve of b
//     needs nothing.  After the launch `done[seq % ring]` is recorded on aux.
//   * An S-lane solve of a batch whose last solve is un-joined on aux first makes S wait on that solve's done event (a ring slot that
//     has been re-recorded since holds a LATER aux solve, which implies the earlier one).
//   * Every other entry point that takes a batch JOINS first (RP_NEED, the single choke point; rp_batch_stream and rp_batch_destroy too):
//     S waits on the newest un-joined done event -- aux is in order, one event suffices -- and the operation counts as S-side work
//     of its batch (dirty_ticket, s_ticket).
// So consecutive solves of different batches overlap pairwise, and whatever a caller can observe through the API or through its own stream
// -- results, events, rp_batch_sync, the stream handle -- is ordered as before.  Foreign work on S cannot conflict: eligible solves touch
// only library-private memory (no bound solution buffer, no raw pointer out); a path that breaks that is excluded, not synchronised.
// The context's mutex is held for the length of an entry point (lane_guard), so tickets are taken in the order the work is enqueued
// also where threads share a stream.  A failed launch leaves the tickets as they were.
// mode 1: the smallest of 65,536 / 262,144 / 1,048,576 problems at which overlapping every eligible solve was not slower than none over 40
// back-to-back solves (1.50x, 1.22x, 1.04x: profiles/solve_overlap_ab.log).  Below it a solve is a few waves per SIMD and unmeasured.
constexpr size_t kOverlapMinProblems = 65536;
constexpr unsigned kDoneRing = 8;

}  // namespace

struct rp_overlap {
    int device;
    hipStream_t S;
    bool own_S;                // a batch created S (rp_batch_create without a stream): destroyed with the last reference
    int refs;                  // under g_overlap_registry_mutex
    std::recursive_mutex mu;   // everything below
    bool lanes_live;           // aux, fork and done[] exist (created at the first solve that may overlap)
    hipStream_t aux;
    hipEvent_t fork, done[kDoneRing];
    uint64_t ticket;           // of the last operation enqueued
    uint64_t dirty_ticket;     // of the last S-side operation that was not an eligible solve
    uint64_t fork_ticket;      // the ticket at which fork was recorded last: S-side operations up to it precede fork
    uint64_t aux_fork_ticket;  // the fork_ticket aux has waited on
    uint64_t aux_seq;          // aux solves enqueued
    uint64_t joined_seq;       // aux solves up to this one precede work S has been made to wait for
    bool after_S_solve;        // the last operation enqueued was an eligible solve on S: the next eligible solve goes to aux
    rp_overlap *next;
};

namespace {

std::mutex g_overlap_registry_mutex;
rp_overlap *g_overlap_registry = nullptr;
std::atomic<int> g_overlap_mode{1};
std::atomic<unsigned long long> g_overlap_stats[4];      // solves sent to aux / kept on S although eligible / joins enqueued / solves excluded

rp_overlap *overlap_acquire(int device, hipStream_t stream, bool own)
{
    std::lock_guard<std::mutex> lock(g_overlap_registry_mutex);
    rp_overlap *c = g_overlap_registry;
    while (c && !(c->device == device && c->S == stream)) c = c->next;
    if (!c) {
        c = new (std::nothrow) rp_overlap();
        if (!c) return nullptr;
        c->device = device;
        c->S = stream;
        c->next = g_overlap_registry;
        g_overlap_registry = c;
    }
    c->own_S = c->own_S || own;
    ++c->refs;
    return c;
}

void overlap_release(rp_overlap *c)
{
    if (!c) return;
    {
        std::lock_guard<std::mutex> lock(g_overlap_registry_mutex);
        if (--c->refs > 0) return;
        rp_overlap **at = &g_overlap_registry;
        while (*at && *at != c) at = &(*at)->next;
        if (*at) *at = c->next;
    }
    if (c->lanes_live) {
        (void)hipStreamSynchronize(c->aux);
        (void)hipStreamDestroy(c->aux);
        (void)hipEventDestroy(c->fork);
        for (unsigned i = 0; i < kDoneRing; ++i) (void)hipEventDestroy(c->done[i]);
    }
    if (c->own_S && c->S) (void)hipStreamDestroy(c->S);
    delete c;
}

// The HIP runtime multiplexes a process's streams onto a handful of hardware queues, and two streams that share one serialise
// (profiles/r6_tuning.md): an auxiliary stream that merely exists can cost a caller who deals work onto streams of its own the queue it
// counted on.  rp_pipeline_create calls this: every context of the device gives its auxiliary stream back, once that has drained.  The
// next solve that may overlap creates it again (need_lanes), and records fork anew.
void overlap_retire_lanes(int device)
{
    std::lock_guard<std::mutex> lock(g_overlap_registry_mutex);
    for (rp_overlap *c = g_overlap_registry; c; c = c->next) {
        if (c->device != device) continue;
        std::lock_guard<std::recursive_mutex> own(c->mu);
        if (!c->lanes_live) continue;
        (void)hipStreamSynchronize(c->aux);      // everything on aux has finished: nothing is left to join
        c->joined_seq = c->aux_seq;
        (void)hipStreamDestroy(c->aux);
        (void)hipEventDestroy(c->fork);
        for (unsigned i = 0; i < kDoneRing; ++i) (void)hipEventDestroy(c->done[i]);
        c->fork_ticket = c->aux_fork_ticket = 0;
        c->lanes_live = false;
    }
}

// holds the context's mutex for the length of an entry point
struct lane_guard {
    rp_overlap *c;
    explicit lane_guard(rp_overlap *c_) : c(c_) { if (c) c->mu.lock(); }
    ~lane_guard() { unlock(); }
    void unlock() { if (c) c->mu.unlock(); c = nullptr; }
    lane_guard(const lane_guard &) = delete;
    lane_guard &operator=(const lane_guard &) = delete;
};

// the join, and the ticket of an operation that goes onto the caller's stream (under the guard)
int on_caller_stream(rp_batch *b)
{
    rp_overlap *c = b->lanes;
    if (!c) return RP_OK;
    if (c->aux_seq > c->joined_seq) {
        RP_HIP(hipStreamWaitEvent(b->stream, c->done[c->aux_seq % kDoneRing], 0));
        if (b->stream == c->S) c->joined_seq = c->aux_seq;
        ++g_overlap_stats[2];
    }
    c->dirty_ticket = b->s_ticket = ++c->ticket;
    c->after_S_solve = false;
    return RP_OK;
}

int need_lanes(rp_overlap *c)
{
    if (c->lanes_live) return RP_OK;
    hipStream_t aux = nullptr;
    hipEvent_t ev[kDoneRing + 1];
    unsigned made = 0;
    hipError_t e = hipStreamCreateWithFlags(&aux, hipStreamNonBlocking);
    if (e != hipSuccess) aux = nullptr;
    for (; e == hipSuccess && made < kDoneRing + 1; ++made) {
        e = hipEventCreateWithFlags(&ev[made], hipEventDisableTiming);
        if (e != hipSuccess) break;
    }
    if (e != hipSuccess) {
        for (unsigned i = 0; i < made; ++i) (void)hipEventDestroy(ev[i]);
        if (aux) (void)hipStreamDestroy(aux);
        return fail(e == hipErrorOutOfMemory ? RP_ERR_NOMEM : RP_ERR_DEVICE, "overlap lanes: %s", hipGetErrorString(e));
    }
    c->aux = aux;
    c->fork = ev[kDoneRing];
    for (unsigned i = 0; i < kDoneRing; ++i) c->done[i] = ev[i];
    c->lanes_live = true;
    return RP_OK;
}

int record_fork(rp_overlap *c)
{
    RP_HIP(hipEventRecord(c->fork, c->S));
    c->fork_ticket = c->ticket;
    return RP_OK;
}

// the lane of an eligible solve of b and the waits ahead of it (the ordering rule above); nothing here takes a ticket
int choose_lane(rp_batch *b, hipStream_t *lane, bool *on_aux)
{
    rp_overlap *c = b->lanes;
    int st = need_lanes(c);
    if (st != RP_OK) return st;
    *on_aux = c->after_S_solve;
    if (*on_aux) {
        if (c->dirty_ticket > c->fork_ticket || b->s_ticket > c->fork_ticket) st = record_fork(c);
        if (st != RP_OK) return st;
        if (c->aux_fork_ticket != c->fork_ticket) {
            RP_HIP(hipStreamWaitEvent(c->aux, c->fork, 0));
            c->aux_fork_ticket = c->fork_ticket;
        }
        *lane = c->aux;
        return RP_OK;
    }
    if (b->aux_seq > c->joined_seq) {
        RP_HIP(hipStreamWaitEvent(c->S, c->done[b->aux_seq % kDoneRing], 0));
        c->joined_seq = b->aux_seq;
        ++g_overlap_stats[2];
    }
    // fork ahead of this solve, for the aux solve that may follow -- unless what dirtied S was work on this very batch (set_problems, solve;
    // restart, solve; ...): in such a per-batch sequence the next solve follows work of its own too and stays on S, and an event per
    // solve is not free (1.5 % of the by-hand loop of bench.py's end_to_end).  Should an aux solve follow after all, it records fork itself.
    if (c->dirty_ticket > c->fork_ticket && b->s_ticket != c->dirty_ticket) st = record_fork(c);
    *lane = c->S;
    return st;
}

// behind a launch that succeeded: its ticket, and on aux its done event
int solve_enqueued(rp_batch *b, bool on_aux)
{
    rp_overlap *c = b->lanes;
    const uint64_t t = ++c->ticket;
    c->after_S_solve = !on_aux;
    if (!on_aux) {
        b->s_ticket = t;
        ++g_overlap_stats[1];
        return RP_OK;
    }
    b->aux_seq = ++c->aux_seq;
    ++g_overlap_stats[0];
    const hipError_t e = hipEventRecord(c->done[b->aux_seq % kDoneRing], c->aux);
    if (e != hipSuccess) {      // no event to wait on: wait here, once
        (void)hipStreamSynchronize(c->aux);
        c->joined_seq = c->aux_seq;
        return fail(RP_ERR_DEVICE, "hipEventRecord: %s", hipGetErrorString(e));
    }
    return RP_OK;
}

// (not a do-while: the guard lives to the end of the entry point)
#define RP_NEED(b)                                              \
    if (!(b)) return fail(RP_ERR_INVALID, "null batch handle"); \
    lane_guard lane_guard_((b)->lanes);                         \
    do {                                                        \
        RP_HIP(hipSetDevice((b)->device));                      \
        const int js_ = on_caller_stream(b);                    \
        if (js_ != RP_OK) return js_;                           \
    } while (0)

// ---- the transitions (the table above the struct) ----
int first_constant(const rp_batch *b) { return 3 + rp::num_constraints(b->view.variant); }      // fields from here on are constants: pos0, vel0, pos1, pos2, vel2
bool is_end_velocity(const rp_batch *b, int field) { return field == first_constant(b) + 1 || field == first_constant(b) + 4; }

// the four events that give the batch a new state differ in five answers; raw pointers to the old state lose their meaning in all of them
void new_state(rp_batch *b, bool scheduled, bool zero_end_vel, bool unpredicted, bool lazy, bool vel_start)
{
    b->view.scheduled = scheduled;
    b->view.zero_end_vel = zero_end_vel;
    b->unpredicted = unpredicted;
    b->at_start = lazy;
    b->records_current = lazy;      // the records are the batch's positions exactly as long as nothing but set_problems has written any
    b->vel_start = vel_start;
    b->raw_state_out = false;
    b->sol_stale = true;
}
void created(rp_batch *b) { b->view.scheduled = false; b->view.zero_end_vel = true; }      // (the struct is zeroed) the state starts all-zero, in problem order
void identical_problems(rp_batch *b) { new_state(b, false, true, false, false, false); }      // nothing to schedule; identical step counts
// the feasible-start rule (vel0 = vel2 = 0): what the order was fitted to
void problems_given(rp_batch *b) { new_state(b, true, true, false, true, false); b->ungated_steps = 0.0; }
// the order was fitted to rest-to-rest starts; the general Newton kernels (bit-identical to the zero-velocity ones where the velocities are 0)
void problems_vel_given(rp_batch *b) { new_state(b, true, false, true, false, true); b->ungated_steps = 0.0; }
void rows_given(rp_batch *b, bool zero_end_vel) { new_state(b, true, zero_end_vel, true, false, false); }      // any state: the order predicts nothing about it

void restarted(rp_batch *b)
{
    b->sol_stale = true;
    if (!b->raw_positions_out) b->unpredicted = false;      // back on the feasible start of the positions the order was computed from
    if (b->at_start) return;                                // still lazy: the start is only written out
    if (b->vel_start) b->unpredicted = true;                // back to the start with the end velocities the batch holds
    else b->view.zero_end_vel = true;
    b->ungated_steps = 0.0;
}

void stepped(rp_batch *b, int k) { b->ungated_steps += (double)k; b->sol_stale = true; }
void moved(rp_batch *b) { b->sol_stale = true; b->unpredicted = true; }
void nudged(rp_batch *b, int field, double delta)
{
    moved(b);
    if (field >= first_constant(b)) b->records_current = false;      // a constant moved: the records no longer are the batch's positions
    if (is_end_velocity(b, field) && delta != 0.0) b->view.zero_end_vel = false;
}

void raw_pointer_out(rp_batch *b, int field)
{
    moved(b);
    b->records_current = false;      // the caller may write through the pointer, now or at any later time
    if (field >= first_constant(b)) b->raw_positions_out = true;
    else b->raw_state_out = true;
    if (is_end_velocity(b, field)) b->view.zero_end_vel = false;      // ... non-zero end velocities the batch never sees: the Newton kernels read vel0X and vel2X
}

void left_lazy_start(rp_batch *b) { b->at_start = false; }     // the start is written out (materialize), or a START launch forms it in registers
void solution_bound(rp_batch *b) { b->sol_stale = true; }        // nothing in the new buffer is current
void solution_current(rp_batch *b) { b->sol_stale = false; }     // a gated launch has been enqueued: it writes the record of every problem it works on

// A batch that has just been given its problems is "at its start" without the start being written: the fused gated solve forms it in
// registers (k_solve_chunks<START>).  Every other consumer of the state goes through here first: positions from the records into the
// constant fields, their feasible start, cleared progress words -- bit for bit what the fused solve starts from.
int materialize(rp_batch *b)
{
    if (!b->at_start) return RP_OK;
    left_lazy_start(b);
    RP_HIP(rp::launch_start_from_records(b->view, b->params, nullptr, nullptr, false, b->stream));      // (the progress counters were zeroed by the scheduling pass)
    return RP_OK;
}

// ---- the questions asked of that state ----
// may this fused solve form its start in registers?  (reference mode only; it then consumes the lazy start)
bool starts_in_registers(const rp_batch *b, int max_iter)
{
    return b->at_start && b->params.mu_mode == 0 && b->params.stall_window == 0 && b->view.zero_end_vel && max_iter > 0;
}

// which form of the fused gated kernel: 0 = plain, 1 = the one that watches for fixed points (a batch whose state has been set, nudged, moved
// or handed out raw: starts outside the feasible set use their budget up at once instead of walking a hundred halvings two hundred times:
// exact), 2..8 = that one in so many rounds (on request: rp_params.handoff_rounds; a batch big enough for a second wave).  Reference mode only.
int gated_rounds(const rp_batch *b, bool from_start, int max_iter)
{
    if (from_start || b->params.mu_mode != 0 || b->params.stall_window > 0 || max_iter <= 0 || b->params.handoff_rounds == -1) return 0;
    const int rounds = b->params.handoff_rounds >= 2 && b->view.n > 64 ? b->params.handoff_rounds : 1;
    return b->unpredicted || rounds > 1 ? rounds : 0;
}

// A gated launch writes the bound solution record of every problem it WORKS ON (k_solve_chunks); problems that finished in an
// earlier launch are skipped without touching their state.  Their records are current only if nothing but gated solves has run
// since they were written: otherwise (a new buffer, steps, a nudge, a set_state ... in between, or a raw pointer to the state out)
// the launch is preceded by one pass that writes every record from the state as it is (k_solution, 68 B per problem).
bool needs_seed(const rp_batch *b) { return b->view.solution && (b->sol_stale || b->raw_state_out); }

// may the plot data of the whole batch go through problem-order records instead of the per-field gather?
bool samples_through_records(const rp_batch *b)
{
    return b->view.scheduled && b->view.zero_end_vel && b->records_current && !b->raw_positions_out && b->view.records;
}

// The protocol around every gated launch: the ungated steps that the records' counts include, the seed (not before a START launch, which
// stores every record itself), the launch, and -- only behind a launch that succeeded, a failed one has written no record -- solution_current().
int before_gated_launch(rp_batch *b, bool seed)
{
    b->view.iters_add = (int)b->ungated_steps;
    if (seed && needs_seed(b)) RP_HIP(rp::launch_solution(b->view, b->view.solution, b->stream));
    return RP_OK;
}

#define RP_NEED_STATE(b)                     \
    RP_NEED(b);                              \
    do {                                     \
        const int ms_ = materialize(b);      \
        if (ms_ != RP_OK) return ms_;        \
    } while (0)

// What every derivative entry (rp_batch_solution_vjp ... rp_batch_solution_jacobian_vel) asks for, in the order it is tested: a
// handle, an F3 batch in double storage (the message names the entry), every output (`outputs`: all of them given), the state
#define RP_NEED_F3_STATE(b, outputs)                                                \
    if (!(b)) return fail(RP_ERR_INVALID, "null batch handle");                     \
    if ((b)->view.variant != RP_VARIANT_F3 || (b)->view.dtype != RP_DTYPE_F64)      \
        return fail(RP_ERR_UNSUPPORTED, "%s: F3 with RP_DTYPE_F64 only", __func__); \
    if (!(outputs)) return fail(RP_ERR_INVALID, "null output");                     \
    RP_NEED_STATE(b)

// The *_range calls (a watched problem, a page of a table) go through one small device buffer that lives as long as
// the batch: kRangeChunk problems x the widest row (the F3 constraint table, 1 + 14 * 8 doubles) = 0.9 MB.
constexpr size_t kRangeChunk = 1024, kRangeRow = 113;

// The solver constants: the one list of the fields that rp_params and rp::HostParams share (the same names on both sides), each with its
// default, the reference's compile-time value (include/rp_batch.h).  A new constant is added here, and to the two structs.
#define RP_PARAMS(X)                                                                                                                  \
    X(accel_limit, 100.0) X(mu_divisor, 10.0) X(boundary_fraction, 0.99) X(backtrack, 0.5) X(armijo, 0.01) X(max_backtracks, 100)     \
    X(stall_window, 0) X(mu_mode, 0) X(mu_sigma_try[0], 0.01) X(mu_sigma_try[1], 0.03) X(handoff_rounds, 0) X(handoff_lanes, 24)

template <typename To, typename From> void copy_params(To &to, const From &from)
{
#define X(field, value) to.field = from.field;
    RP_PARAMS(X)
#undef X
}

rp::HostParams default_params()
{
    rp::HostParams hp;
#define X(field, value) hp.field = value;
    RP_PARAMS(X)
#undef X
    return hp;
}

int reset_progress(rp_batch *b)
{
    b->ungated_steps = 0.0;
    RP_HIP(rp::launch_clear_progress(b->view, b->stream));
    return RP_OK;
}

// the scheduled order from positions given as three strided double arrays in problem order (device memory), on the batch's
// own stream (three small kernels of ours, schedule.hip; round 2's library sort needed a queue of its own).
// The caller applies its transition once this has succeeded.
int schedule(rp_batch *b, const double *d_pos0, const double *d_pos1, const double *d_pos2, size_t pstride, bool write_positions)
{
    if (!b->d_sched) {
        RP_HIP(rp::schedule_scratch_bytes(b->view.n, &b->sched_bytes));
        RP_HIP(hipMalloc(&b->d_sched, b->sched_bytes));
    }
    // 32 B per problem: what the scheduling pass keeps for the feasible start / the fused solve
    if (write_positions && !b->view.records) RP_HIP(hipMalloc((void **)&b->view.records, b->view.n * sizeof(rp::StartRecord)));
    RP_HIP(rp::launch_schedule(b->view, d_pos0, d_pos1, d_pos2, pstride, write_positions, b->d_sched, b->sched_bytes, b->stream, b->slim_schedule));
    return RP_OK;
}

// host position arrays into d_pos (3 n doubles: pos0, pos1, pos2), in stream order
int stage_positions(rp_batch *b, const double *pos0, const double *pos1, const double *pos2)
{
    if (!pos0 || !pos1 || !pos2) return fail(RP_ERR_INVALID, "null position array");
    const size_t n = b->view.n;
    if (!b->d_pos) RP_HIP(hipMalloc((void **)&b->d_pos, 3 * n * sizeof(double)));
    RP_HIP(hipMemcpyAsync(b->d_pos, pos0, n * sizeof(double), hipMemcpyHostToDevice, b->stream));
    RP_HIP(hipMemcpyAsync(b->d_pos + n, pos1, n * sizeof(double), hipMemcpyHostToDevice, b->stream));
    RP_HIP(hipMemcpyAsync(b->d_pos + 2 * n, pos2, n * sizeof(double), hipMemcpyHostToDevice, b->stream));
    return RP_OK;
}

// the four doubles of the last rp_batch_reduce_device into d_scratch + 4096, read back through pinned memory
int read_summary(rp_batch *b, rp_reduction *out)
{
    double *h = reinterpret_cast<double *>(b->h_pinned + 64);
    RP_HIP(hipMemcpyAsync(h, b->d_scratch + 4096, 4 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    RP_HIP(hipStreamSynchronize(b->stream));
    out->max_residual_sq = h[0];
    out->max_gap = h[1];
    out->n_converged = h[2];
    out->total_steps = h[3];
    return RP_OK;
}

int need_words(rp_batch *b)
{
    if (!b->d_words) RP_HIP(hipMalloc((void **)&b->d_words, 2 * b->view.n * sizeof(uint32_t)));
    return RP_OK;
}

int need_aos(rp_batch *b)
{
    if (!b->d_aos) RP_HIP(hipMalloc((void **)&b->d_aos, b->view.n * rp::state_len(b->view.variant) * sizeof(double)));
    return RP_OK;
}

int check_range(const rp_batch *b, size_t first, size_t count, const void *out)
{
    if (!out) return fail(RP_ERR_INVALID, "null output");
    if (first > b->view.n || count > b->view.n - first) return fail(RP_ERR_INVALID, "range [%zu, %zu + %zu) outside the batch of %zu", first, first, count, b->view.n);
    return RP_OK;
}

// A *_range read-back: problems [first, first + count) in chunks of kRangeChunk through d_range.  produce(first, count) enqueues the
// kernel that fills the staging buffer, copy_out(done, count) the copies of that chunk to the caller's arrays.
template <typename Produce, typename CopyOut> int read_range(rp_batch *b, size_t first, size_t count, Produce produce, CopyOut copy_out)
{
    if (!b->d_range) RP_HIP(hipMalloc((void **)&b->d_range, kRangeChunk * kRangeRow * sizeof(double)));
    for (size_t done = 0; done < count; done += kRangeChunk) {
        const size_t c = count - done < kRangeChunk ? count - done : kRangeChunk;
        RP_HIP(produce(first + done, c));
        RP_HIP(copy_out(done, c));
        RP_HIP(hipStreamSynchronize(b->stream));      // the staging buffer is reused by the next chunk
    }
    return RP_OK;
}

int check_steps(int k) { return k < 0 || k > 1000000 ? fail(RP_ERR_INVALID, "step count %d out of range (0..1000000)", k) : RP_OK; }
int check_max_iter(int max_iter) { return max_iter < 0 || max_iter > 1000000 ? fail(RP_ERR_INVALID, "max_iter %d out of range (0..1000000)", max_iter) : RP_OK; }
int check_gap_tol(double gap_tol) { return gap_tol == gap_tol ? RP_OK : fail(RP_ERR_INVALID, "gap_tol is NaN"); }

}  // namespace

extern "C" {

const char *rp_version(void) { return "rocket_path_amd 0.6 (gfx950)"; }
int rp_abi_version(void) { return RP_ABI_VERSION; }
size_t rp_params_size(void) { return sizeof(rp_params); }
const char *rp_last_error(void) { return g_err; }

const char *rp_status_string(int status)
{
    switch (status) {
    case RP_OK: return "ok";
    case RP_ERR_INVALID: return "invalid argument";
    case RP_ERR_DEVICE: return "HIP error";
    case RP_ERR_NOMEM: return "out of memory";
    case RP_ERR_UNSUPPORTED: return "unsupported";
    case RP_ERR_NO_DEVICE: return "no HIP device (this path has no CPU fallback)";
    default: return "unknown status";
    }
}

int rp_device_count(int *count)
{
    if (!count) return fail(RP_ERR_INVALID, "count is null");
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess) { *count = 0; (void)hipGetLastError(); return fail(RP_ERR_NO_DEVICE, "hipGetDeviceCount: %s", hipGetErrorString(e)); }
    *count = n;
    return RP_OK;
}

int rp_device_id(int device, char *out, size_t len)
{
    if (!out || len < 64) return fail(RP_ERR_INVALID, "rp_device_id needs a buffer of at least 64 bytes");
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n == 0) { (void)hipGetLastError(); return fail(RP_ERR_NO_DEVICE, "no HIP device visible"); }
    if (device < 0 || device >= n) return fail(RP_ERR_INVALID, "device %d out of range (%d visible)", device, n);
    char bus[32] = "";
    RP_HIP(hipDeviceGetPCIBusId(bus, (int)sizeof bus, device));
    hipUUID uuid;
    std::memset(&uuid, 0, sizeof uuid);
    char hex[2 * sizeof uuid.bytes + 1] = "";
    if (hipDeviceGetUuid(&uuid, device) == hipSuccess) {
        for (size_t i = 0; i < sizeof uuid.bytes; ++i) snprintf(hex + 2 * i, 3, "%02x", (unsigned)(unsigned char)uuid.bytes[i]);
    } else {
        (void)hipGetLastError();
    }
    snprintf(out, len, "pci %s uuid %s", bus, hex[0] ? hex : "?");
    return RP_OK;
}

void rp_params_default(rp_params *p)
{
    if (p) copy_params(*p, default_params());
}

int rp_batch_create(rp_batch **out, int variant, int dtype, size_t n, int device, void *stream)
{
    if (!out) return fail(RP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (variant != RP_VARIANT_F3 && variant != RP_VARIANT_F4) return fail(RP_ERR_INVALID, "variant %d (want 3 or 4)", variant);
    if (dtype != RP_DTYPE_F64 && dtype != RP_DTYPE_F32 && dtype != RP_DTYPE_F32_STATE)
        return fail(RP_ERR_INVALID, "dtype %d (want 0 = f64, 1 = f32 or 2 = f32 state with f64 arithmetic)", dtype);
    if (n == 0) return fail(RP_ERR_INVALID, "empty batch");
    if (n > 0x7fffffffu) return fail(RP_ERR_INVALID, "batch of %zu problems (at most 2^31 - 1 per batch; shard larger jobs)", n);
    int count = 0;
    int st = rp_device_count(&count);
    if (st != RP_OK || count == 0) return fail(RP_ERR_NO_DEVICE, "no HIP device visible; the interior-point path runs on the GPU only");
    if (device < 0 || device >= count) return fail(RP_ERR_INVALID, "device %d out of range (%d visible)", device, count);
    RP_HIP(hipSetDevice(device));

    rp_batch *b = new (std::nothrow) rp_batch();
    if (!b) return fail(RP_ERR_NOMEM, "host allocation failed");
    std::memset(b, 0, sizeof *b);
    b->device = device;
    b->params = default_params();
    b->view.n = n;
    b->view.variant = variant;
    b->view.dtype = dtype;
    // Field f of problem i lives at base + f * stride + i.  A stride that is a large power of two in bytes (8 MiB at
    // n = 2^20 doubles) puts element i of all 16 fields on the same HBM channel and bank: the 25 streams of a step then
    // fight over one row buffer (measured, profiles/probes/stride_probe.py: 3.7 TB/s at k = 1 against 4.6 TB/s with the
    // fields 1.25 KiB or more out of phase; plateau from there on).  So the stride is an ODD multiple of 512 elements.
    b->view.stride = (n + 511) / 512 * 512;
    if ((b->view.stride / 512) % 2 == 0) b->view.stride += 512;
#ifdef RP_TUNING      // tuning builds only (profiles/probes/stride_probe.py): the shipped library reads nothing from the environment
    if (const char *pad = getenv("RP_STRIDE_PAD")) b->view.stride += (size_t)atoi(pad) / 16 * 16;
#endif
    created(b);
    const size_t fields = (size_t)rp::state_len(variant);

    hipError_t e = hipSuccess;
    if (stream) { b->stream = (hipStream_t)stream; b->own_stream = false; }
    else { e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking); b->own_stream = (e == hipSuccess); }
    if (e == hipSuccess && !(b->lanes = overlap_acquire(device, b->stream, b->own_stream))) e = hipErrorOutOfMemory;      // (the context now owns a stream created here)
    lane_guard guard(b->lanes);
    if (e == hipSuccess) e = hipMalloc(&b->view.base, fields * b->view.stride * rp::storage_size(dtype));
    if (e == hipSuccess) e = hipMalloc((void **)&b->view.iters, n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&b->view.status, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&b->view.slot_of, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&b->view.prob_of, n * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc((void **)&b->view.counters, 128 * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void **)&b->d_scratch, (4096 + 4) * sizeof(double));
    if (e == hipSuccess) e = hipHostMalloc((void **)&b->h_pinned, 72 * sizeof(unsigned long long), hipHostMallocDefault);
    if (e == hipSuccess) e = hipMemsetAsync(b->view.base, 0, fields * b->view.stride * rp::storage_size(dtype), b->stream);
    if (e == hipSuccess) e = rp::launch_clear_progress(b->view, b->stream);
    if (e != hipSuccess) {
        const int code = fail(e == hipErrorOutOfMemory ? RP_ERR_NOMEM : RP_ERR_DEVICE, "rp_batch_create: %s", hipGetErrorString(e));
        guard.unlock();
        rp_batch_destroy(b);
        return code;
    }
    st = on_caller_stream(b);      // the clearing above is S-side work of this batch
    if (st != RP_OK) {
        guard.unlock();
        rp_batch_destroy(b);
        return st;
    }
    *out = b;
    return RP_OK;
}

int rp_batch_destroy(rp_batch *b)
{
    if (!b) return RP_OK;
    (void)hipSetDevice(b->device);
    {
        // join, synchronise as ever, and aux too if this batch has work pending there (its memory is freed below)
        lane_guard guard(b->lanes);
        const bool on_aux = b->lanes && b->lanes->lanes_live && b->aux_seq > b->lanes->joined_seq;
        if (b->stream) (void)on_caller_stream(b);
        if (b->stream) (void)hipStreamSynchronize(b->stream);
        if (on_aux) (void)hipStreamSynchronize(b->lanes->aux);
    }
    for (int i = 0; i < 8; ++i) if (b->event_live[i]) (void)hipEventDestroy(b->events[i]);
    if (b->view.base) (void)hipFree(b->view.base);
    if (b->view.iters) (void)hipFree(b->view.iters);
    if (b->view.status) (void)hipFree(b->view.status);
    if (b->view.slot_of) (void)hipFree(b->view.slot_of);
    if (b->view.prob_of) (void)hipFree(b->view.prob_of);
    if (b->view.records) (void)hipFree(b->view.records);
    if (b->view.lists) (void)hipFree(b->view.lists);
    if (b->d_words) (void)hipFree(b->d_words);
    if (b->d_sched) (void)hipFree(b->d_sched);
    if (b->view.counters) (void)hipFree(b->view.counters);
    if (b->d_scratch) (void)hipFree(b->d_scratch);
    if (b->h_pinned) (void)hipHostFree(b->h_pinned);
    if (b->d_aos) (void)hipFree(b->d_aos);
    if (b->d_pos) (void)hipFree(b->d_pos);
    if (b->d_range) (void)hipFree(b->d_range);
    if (b->d_solscratch) (void)hipFree(b->d_solscratch);
    if (b->lanes) overlap_release(b->lanes);      // the last batch on the stream destroys aux, the events and a stream a batch created
    else if (b->own_stream && b->stream) (void)hipStreamDestroy(b->stream);
    delete b;
    return RP_OK;
}

int rp_batch_set_params(rp_batch *b, const rp_params *p)
{
    if (!b || !p) return fail(RP_ERR_INVALID, "null argument");
    if (!(p->accel_limit > 0) || !(p->mu_divisor > 0) || !(p->boundary_fraction > 0 && p->boundary_fraction <= 1) ||
        !(p->backtrack > 0 && p->backtrack < 1) || !(p->armijo >= 0 && p->armijo < 1) || p->max_backtracks < 0 ||
        p->max_backtracks > 4096 || p->stall_window < 0)      // every device loop must stay short: a runaway kernel takes the GPU with it
        return fail(RP_ERR_INVALID, "parameter out of range");
    if (p->mu_mode != 0 && p->mu_mode != 1) return fail(RP_ERR_INVALID, "mu_mode %d (want 0 = reference or 1 = centring by trial)", p->mu_mode);
    if (!(p->handoff_rounds == 0 || p->handoff_rounds == -1 || (p->handoff_rounds >= 2 && p->handoff_rounds <= 8)))
        return fail(RP_ERR_INVALID, "handoff_rounds %d (want 0 = automatic, -1 = never, or 2..8)", p->handoff_rounds);
    if (p->handoff_lanes < 1 || p->handoff_lanes > 48) return fail(RP_ERR_INVALID, "handoff_lanes %d (want 1..48)", p->handoff_lanes);
    if (p->mu_mode == 1) {
        if (b->view.dtype == RP_DTYPE_F32) return fail(RP_ERR_UNSUPPORTED, "mu_mode 1 needs double arithmetic (RP_DTYPE_F64 or RP_DTYPE_F32_STATE)");
        if (!(p->mu_sigma_try[0] > 0 && p->mu_sigma_try[0] <= p->mu_sigma_try[1] && p->mu_sigma_try[1] < 1))
            return fail(RP_ERR_INVALID, "mu_sigma_try must satisfy 0 < [0] <= [1] < 1");
    }
    if (b->at_start && p->accel_limit != b->params.accel_limit) {
        // the feasible start of a batch that has just been given its problems is formed lazily, from the limit of the moment the
        // problems were set: write it out before the limit changes (set_problems, set_params, solve = the start of the OLD limit,
        // as if set_problems had written it)
        RP_NEED_STATE(b);
    }
    copy_params(b->params, *p);
    return RP_OK;
}

int rp_batch_get_params(const rp_batch *b, rp_params *p)
{
    if (!b || !p) return fail(RP_ERR_INVALID, "null argument");
    copy_params(*p, b->params);
    return RP_OK;
}

int rp_batch_size(const rp_batch *b, size_t *n)
{
    if (!b || !n) return fail(RP_ERR_INVALID, "null argument");
    *n = b->view.n;
    return RP_OK;
}

int rp_batch_info(const rp_batch *b, int *variant, int *dtype, int *device)
{
    if (!b) return fail(RP_ERR_INVALID, "null batch handle");
    if (variant) *variant = b->view.variant;
    if (dtype) *dtype = b->view.dtype;
    if (device) *device = b->device;
    return RP_OK;
}

// every problem of the batch in the one state `s` (state_len values)
static int init_identical(rp_batch *b, const double *s)
{
    RP_HIP(rp::launch_init_const(b->view, s, b->stream));
    identical_problems(b);
    return reset_progress(b);
}

// initDefault: pos (0, 200, 400), zero velocities, durations 3.5, multipliers 1
// (onedpath_ip.cpp:201-228, onedpath2_ip.cpp:164-193).
int rp_batch_init_default(rp_batch *b)
{
    RP_NEED(b);
    double s[16];
    const int m = rp::num_constraints(b->view.variant);
    s[0] = 0.0; s[1] = 3.5; s[2] = 3.5;
    for (int i = 0; i < m; ++i) s[3 + i] = 1.0;
    s[3 + m + 0] = 0.0; s[3 + m + 1] = 0.0; s[3 + m + 2] = 200.0; s[3 + m + 3] = 400.0; s[3 + m + 4] = 0.0;
    return init_identical(b, s);
}

// initStuck, onedpath_ip.cpp:177-199.
int rp_batch_init_stuck(rp_batch *b)
{
    RP_NEED(b);
    if (b->view.variant != RP_VARIANT_F3) return fail(RP_ERR_UNSUPPORTED, "the stuck state exists for F3 only (onedpath_ip.cpp:177-199)");
    const double s[16] = {-9.66825, 4.78149, 4.38968,
                          5.45948e-07, 0.00310769, 3.49109e-08, 0.00281523, 8.39344e-07, 1.76937e-06, 0.0187559, 8.42414e-07,
                          0.0, 0.0, 350.0, 400.0, 0.0};
    return init_identical(b, s);
}

// Where each problem goes (scheduled order), its positions copied into its record, progress counters zeroed: three
// kernels (schedule.hip).  The feasible start itself is not written: a fused gated solve that follows forms it in registers,
// anything else materialises it first (materialize above).  The position arrays are consumed in stream order, here.
int rp_batch_set_problems_device(rp_batch *b, const double *d_pos0, const double *d_pos1, const double *d_pos2)
{
    RP_NEED(b);
    if (!d_pos0 || !d_pos1 || !d_pos2) return fail(RP_ERR_INVALID, "null position array");
    if (!b->view.zero_end_vel) {       // a set_state / nudge / field_ptr may have left non-zero end velocities: the start rule zeroes them
        const size_t es = rp::storage_size(b->view.dtype), cb = (size_t)first_constant(b);
        RP_HIP(hipMemsetAsync((char *)b->view.base + (cb + 1) * b->view.stride * es, 0, b->view.n * es, b->stream));
        RP_HIP(hipMemsetAsync((char *)b->view.base + (cb + 4) * b->view.stride * es, 0, b->view.n * es, b->stream));
    }
    int st = schedule(b, d_pos0, d_pos1, d_pos2, 1, true);
    if (st != RP_OK) return st;
    problems_given(b);
    return RP_OK;
}

// The same scheduling pass on the positions, then the start with the velocities written out at once (it writes both velocity fields):
// the fused solve forms only the rest-to-rest start in registers.
int rp_batch_set_problems_vel_device(rp_batch *b, const double *d_pos0, const double *d_pos1, const double *d_pos2,
                                     const double *d_vel0, const double *d_vel2)
{
    RP_NEED(b);
    if (!d_pos0 || !d_pos1 || !d_pos2) return fail(RP_ERR_INVALID, "null position array");
    int st = schedule(b, d_pos0, d_pos1, d_pos2, 1, true);
    if (st != RP_OK) return st;
    problems_vel_given(b);
    RP_HIP(rp::launch_start_from_records(b->view, b->params, d_vel0, d_vel2, true, b->stream));
    return RP_OK;
}

int rp_batch_restart(rp_batch *b)
{
    RP_NEED(b);
    const bool lazy = b->at_start, vel = b->vel_start;
    restarted(b);
    if (lazy) return materialize(b);      // already at the start of its positions: write it out
    RP_HIP(rp::launch_restart(b->view, b->params, vel, b->stream));      // vel: back to the start with the end velocities the batch holds
    RP_HIP(rp::launch_clear_progress(b->view, b->stream));      // the positions have not changed: the scheduled order stays as it is
    return RP_OK;
}

int rp_batch_set_problems(rp_batch *b, const double *pos0, const double *pos1, const double *pos2)
{
    RP_NEED(b);
    int st = stage_positions(b, pos0, pos1, pos2);
    if (st == RP_OK) st = rp_batch_set_problems_device(b, b->d_pos, b->d_pos + b->view.n, b->d_pos + 2 * b->view.n);
    if (st != RP_OK) return st;
    RP_HIP(hipStreamSynchronize(b->stream));   // the host arrays may be reused on return
    return RP_OK;
}

int rp_batch_set_problems_vel(rp_batch *b, const double *pos0, const double *pos1, const double *pos2, const double *vel0, const double *vel2)
{
    RP_NEED(b);
    int st = stage_positions(b, pos0, pos1, pos2);
    if (st != RP_OK) return st;
    const size_t n = b->view.n;
    double *d_vel = nullptr;      // the two velocity arrays, staged for this call only
    if (vel0 || vel2) RP_HIP(hipMalloc((void **)&d_vel, 2 * n * sizeof(double)));
    hipError_t e = hipSuccess;
    if (vel0) e = hipMemcpyAsync(d_vel, vel0, n * sizeof(double), hipMemcpyHostToDevice, b->stream);
    if (e == hipSuccess && vel2) e = hipMemcpyAsync(d_vel + n, vel2, n * sizeof(double), hipMemcpyHostToDevice, b->stream);
    st = e == hipSuccess ? rp_batch_set_problems_vel_device(b, b->d_pos, b->d_pos + n, b->d_pos + 2 * n, vel0 ? d_vel : nullptr,
                                                            vel2 ? d_vel + n : nullptr)
                         : fail(RP_ERR_DEVICE, "rp_batch_set_problems_vel: %s", hipGetErrorString(e));
    const hipError_t se = hipStreamSynchronize(b->stream);      // the host arrays may be reused on return, the staging freed
    if (d_vel) (void)hipFree(d_vel);
    if (st != RP_OK) return st;
    RP_HIP(se);
    return RP_OK;
}

int rp_batch_set_state(rp_batch *b, const double *aos)
{
    RP_NEED(b);
    if (!aos) return fail(RP_ERR_INVALID, "null state array");
    int st = need_aos(b);
    if (st != RP_OK) return st;
    const size_t M = (size_t)rp::state_len(b->view.variant), bytes = b->view.n * M * sizeof(double), cb = (size_t)first_constant(b);
    bool zero = true;      // which instantiation the Newton kernels may use: are all end velocities zero?  (NaN counts as non-zero)
    for (size_t i = 0; i < b->view.n && zero; ++i) zero = (aos[i * M + cb + 1] == 0.0) && (aos[i * M + cb + 4] == 0.0);
    RP_HIP(hipMemcpyAsync(b->d_aos, aos, bytes, hipMemcpyHostToDevice, b->stream));
    // schedule by the positions in the rows (columns pos0, pos1, pos2 of the reference's enum), then scatter the rows: they are the state
    st = schedule(b, b->d_aos + cb + 0, b->d_aos + cb + 2, b->d_aos + cb + 3, M, false);
    if (st != RP_OK) return st;
    rows_given(b, zero);
    RP_HIP(rp::launch_aos_to_soa(b->view, b->d_aos, b->stream));
    st = reset_progress(b);
    if (st != RP_OK) return st;
    RP_HIP(hipStreamSynchronize(b->stream));
    return RP_OK;
}

int rp_batch_get_state(rp_batch *b, double *aos)
{
    RP_NEED_STATE(b);
    if (!aos) return fail(RP_ERR_INVALID, "null state array");
    int st = need_aos(b);
    if (st != RP_OK) return st;
    const size_t bytes = b->view.n * rp::state_len(b->view.variant) * sizeof(double);
    RP_HIP(rp::launch_soa_to_aos(b->view, b->d_aos, b->stream));
    RP_HIP(hipMemcpyAsync(aos, b->d_aos, bytes, hipMemcpyDeviceToHost, b->stream));
    RP_HIP(hipStreamSynchronize(b->stream));
    return RP_OK;
}

int rp_batch_get_state_range(rp_batch *b, size_t first, size_t count, double *aos)
{
    RP_NEED_STATE(b);
    const int st = check_range(b, first, count, aos);
    if (st != RP_OK) return st;
    const size_t M = (size_t)rp::state_len(b->view.variant);
    return read_range(b, first, count,
                      [&](size_t f, size_t c) { return rp::launch_soa_to_aos_range(b->view, f, c, b->d_range, b->stream); },
                      [&](size_t done, size_t c) { return hipMemcpyAsync(aos + done * M, b->d_range, c * M * sizeof(double), hipMemcpyDeviceToHost, b->stream); });
}

int rp_batch_nudge(rp_batch *b, int var_index, double delta)
{
    RP_NEED_STATE(b);
    if (var_index < 0 || var_index >= rp::state_len(b->view.variant)) return fail(RP_ERR_INVALID, "variable index %d out of range", var_index);
    RP_HIP(rp::launch_nudge(b->view, var_index, delta, b->stream));
    nudged(b, var_index, delta);
    return RP_OK;
}

int rp_batch_step(rp_batch *b, int k)
{
    RP_NEED_STATE(b);
    const int st = check_steps(k);
    if (st != RP_OK || k == 0) return st;
    RP_HIP(rp::launch_steps(b->view, b->params, k, b->stream));
    stepped(b, k);
    return RP_OK;
}

int rp_batch_traffic_probe(rp_batch *b)
{
    RP_NEED_STATE(b);
    RP_HIP(rp::launch_steps(b->view, b->params, 0, b->stream));      // the k = 1 kernel with no steps: its loads and stores, nothing else
    return RP_OK;
}

int rp_batch_step_counted(rp_batch *b, int k, uint32_t *feas_halvings, uint32_t *resid_halvings)
{
    RP_NEED_STATE(b);
    const int st = check_steps(k);
    if (st != RP_OK) return st;
    if (!feas_halvings || !resid_halvings) return fail(RP_ERR_INVALID, "null output");
    if (b->params.mu_mode != 0) return fail(RP_ERR_UNSUPPORTED, "the counted step exists for the reference's mu mode only");
    const size_t n = b->view.n;
    uint32_t *d = nullptr;
    RP_HIP(hipMalloc((void **)&d, 4 * n * sizeof(uint32_t)));
    hipError_t e = rp::launch_steps_counted(b->view, b->params, k, d, d + n, b->stream);
    const uint32_t *out_f = d, *out_r = d + n;
    if (b->view.scheduled) {      // the kernel counts per position: bring the counts into problem order
        if (e == hipSuccess) e = rp::launch_gather_u32(b->view, d, d + 2 * n, b->stream);
        if (e == hipSuccess) e = rp::launch_gather_u32(b->view, d + n, d + 3 * n, b->stream);
        out_f = d + 2 * n;
        out_r = d + 3 * n;
    }
    if (e == hipSuccess) e = hipMemcpyAsync(feas_halvings, out_f, n * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(resid_halvings, out_r, n * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(RP_ERR_DEVICE, "rp_batch_step_counted: %s", hipGetErrorString(e));
    stepped(b, k);
    return RP_OK;
}

int rp_batch_solve(rp_batch *b, double gap_tol, int max_iter, int steps_per_launch)
{
    if (!b) return fail(RP_ERR_INVALID, "null batch handle");
    lane_guard guard(b->lanes);
    RP_HIP(hipSetDevice(b->device));
    int st = check_max_iter(max_iter);
    if (st == RP_OK) st = check_gap_tol(gap_tol);
    if (st != RP_OK) return st;
    const bool fused = steps_per_launch <= 0, from_start = fused && starts_in_registers(b, max_iter);
    const int rounds = fused ? gated_rounds(b, from_start, max_iter) : 0;
    // The eligibility list of the overlap (the ordering rule above RP_NEED): one fused launch that touches library-private memory only.
    // A bound solution buffer and a raw pointer out are the caller's memory or the caller's writes: such a solve stays in S's order.
    const int mode = g_overlap_mode.load(std::memory_order_relaxed);
    const bool eligible = fused && rounds <= 1 && !b->view.solution && !b->raw_state_out && !b->raw_positions_out && !b->pipelined && b->lanes;
    const bool overlapped = mode != 0 && eligible && (mode == 2 || b->view.n >= kOverlapMinProblems);
    if (mode != 0 && !overlapped) ++g_overlap_stats[eligible ? 1 : 3];
    // anything but an overlapped solve joins and is S-side work, as under RP_NEED; so is a start that has to be written out first
    if (!overlapped || (!from_start && b->at_start)) st = on_caller_stream(b);
    if (st != RP_OK) return st;
    if (from_start) left_lazy_start(b);
    else st = materialize(b);
    if (st == RP_OK) st = before_gated_launch(b, !from_start);
    if (st != RP_OK) return st;
    if (fused) {      // every problem to its gate in one launch (or one per round)
        hipStream_t lane = b->stream;
        bool on_aux = false;
        if (overlapped) st = choose_lane(b, &lane, &on_aux);
        if (st != RP_OK) return st;
        if (rounds > 0) {
            if (rounds > 1 && !b->view.lists) RP_HIP(hipMalloc((void **)&b->view.lists, (2 * b->view.n + 16) * sizeof(uint32_t)));
            RP_HIP(rp::launch_solve_rounds(b->view, b->params, gap_tol, max_iter, rounds, b->params.handoff_lanes, 1, lane));
        } else {
            RP_HIP(rp::launch_solve_fused(b->view, b->params, gap_tol, max_iter, from_start, lane));
        }
        if (overlapped) st = solve_enqueued(b, on_aux);
        if (st != RP_OK) return st;
        solution_current(b);
        return RP_OK;
    }
    // bounded host loop: every launch either finishes a problem or advances it by >= 1 step
    const int max_launches = max_iter / steps_per_launch + 2;
    for (int l = 0; l < max_launches; ++l) {
        RP_HIP(rp::launch_solve(b->view, b->params, steps_per_launch, gap_tol, max_iter, b->stream));
        solution_current(b);
        RP_HIP(hipMemcpyAsync(b->h_pinned, b->view.counters, 64 * sizeof(unsigned long long), hipMemcpyDeviceToHost, b->stream));
        RP_HIP(hipStreamSynchronize(b->stream));
        unsigned long long open = 0;
        for (int i = 0; i < 64; ++i) open += b->h_pinned[i];
        if (open == 0) break;
    }
    return RP_OK;
}

int rp_batch_solve_launch(rp_batch *b, double gap_tol, int max_iter, int k)
{
    RP_NEED_STATE(b);
    int st = check_max_iter(max_iter);
    if (st == RP_OK && (k < 1 || k > 1000000)) st = fail(RP_ERR_INVALID, "steps per launch %d out of range (1..1000000)", k);
    if (st == RP_OK) st = check_gap_tol(gap_tol);
    if (st == RP_OK) st = before_gated_launch(b, true);
    if (st != RP_OK) return st;
    RP_HIP(rp::launch_solve(b->view, b->params, k, gap_tol, max_iter, b->stream));
    solution_current(b);
    return RP_OK;
}

int rp_batch_move_toward_feasibility(rp_batch *b)
{
    RP_NEED_STATE(b);
    RP_HIP(rp::launch_move_toward_feasibility(b->view, b->params, b->stream));
    moved(b);
    return RP_OK;
}

int rp_batch_get_iters(rp_batch *b, int32_t *iters, uint32_t *status)
{
    RP_NEED_STATE(b);
    const size_t n = b->view.n;
    const uint32_t *src_it = reinterpret_cast<const uint32_t *>(b->view.iters), *src_st = b->view.status;
    if (b->view.scheduled) {      // the words lie in batch order
        int st = need_words(b);
        if (st != RP_OK) return st;
        if (iters) RP_HIP(rp::launch_gather_u32(b->view, src_it, b->d_words, b->stream));
        if (status) RP_HIP(rp::launch_gather_u32(b->view, src_st, b->d_words + n, b->stream));
        src_it = b->d_words;
        src_st = b->d_words + n;
    }
    if (iters) RP_HIP(hipMemcpyAsync(iters, src_it, n * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream));
    if (status) RP_HIP(hipMemcpyAsync(status, src_st, n * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    RP_HIP(hipStreamSynchronize(b->stream));
    if (iters && b->ungated_steps > 0) {
        const int32_t add = (int32_t)b->ungated_steps;
        for (size_t i = 0; i < n; ++i) iters[i] += add;
    }
    return RP_OK;
}

int rp_batch_solution_device(rp_batch *b, rp_solution *d_out)
{
    RP_NEED_STATE(b);
    if (!d_out) return fail(RP_ERR_INVALID, "null output");
    if (((uintptr_t)d_out & 31u) != 0) return fail(RP_ERR_INVALID, "solution records must be 32-byte aligned");
    b->view.iters_add = (int)b->ungated_steps;
    RP_HIP(rp::launch_solution(b->view, reinterpret_cast<rp::Solution *>(d_out), b->stream));
    return RP_OK;
}

int rp_batch_solution_vjp(rp_batch *b, const double *d_g_vel1, const double *d_g_dur0, const double *d_g_dur1,
                          double *d_pos0_bar, double *d_pos1_bar, double *d_pos2_bar)
{
    RP_NEED_F3_STATE(b, d_pos0_bar && d_pos1_bar && d_pos2_bar);
    RP_HIP(rp::launch_solution_vjp(b->view, b->params, d_g_vel1, d_g_dur0, d_g_dur1, d_pos0_bar, d_pos1_bar, d_pos2_bar, b->stream));
    return RP_OK;
}

int rp_batch_solution_jvp(rp_batch *b, const double *d_t_pos0, const double *d_t_pos1, const double *d_t_pos2,
                          double *d_t_vel1, double *d_t_dur0, double *d_t_dur1)
{
    RP_NEED_F3_STATE(b, d_t_vel1 && d_t_dur0 && d_t_dur1);
    RP_HIP(rp::launch_solution_jvp(b->view, b->params, d_t_pos0, d_t_pos1, d_t_pos2, d_t_vel1, d_t_dur0, d_t_dur1, b->stream));
    return RP_OK;
}

int rp_batch_solution_jacobian(rp_batch *b, double *d_jac)
{
    RP_NEED_F3_STATE(b, d_jac);
    RP_HIP(rp::launch_solution_jacobian(b->view, b->params, d_jac, b->stream));
    return RP_OK;
}

int rp_batch_solution_hessian(rp_batch *b, double *d_jac, double *d_hess)
{
    RP_NEED_F3_STATE(b, d_hess);
    RP_HIP(rp::launch_solution_hessian(b->view, b->params, d_jac, d_hess, b->stream));
    return RP_OK;
}

int rp_batch_solution_vjp_vel(rp_batch *b, const double *d_g_vel1, const double *d_g_dur0, const double *d_g_dur1, double *d_pos0_bar,
                              double *d_pos1_bar, double *d_pos2_bar, double *d_vel0_bar, double *d_vel2_bar)
{
    RP_NEED_F3_STATE(b, d_pos0_bar && d_pos1_bar && d_pos2_bar && d_vel0_bar && d_vel2_bar);
    RP_HIP(rp::launch_solution_vjp_vel(b->view, b->params, d_g_vel1, d_g_dur0, d_g_dur1, d_pos0_bar, d_pos1_bar, d_pos2_bar, d_vel0_bar,
                                       d_vel2_bar, b->stream));
    return RP_OK;
}

int rp_batch_solution_jvp_vel(rp_batch *b, const double *d_t_pos0, const double *d_t_pos1, const double *d_t_pos2, const double *d_t_vel0,
                              const double *d_t_vel2, double *d_t_vel1, double *d_t_dur0, double *d_t_dur1)
{
    RP_NEED_F3_STATE(b, d_t_vel1 && d_t_dur0 && d_t_dur1);
    RP_HIP(rp::launch_solution_jvp_vel(b->view, b->params, d_t_pos0, d_t_pos1, d_t_pos2, d_t_vel0, d_t_vel2, d_t_vel1, d_t_dur0, d_t_dur1,
                                       b->stream));
    return RP_OK;
}

int rp_batch_solution_jacobian_vel(rp_batch *b, double *d_jac)
{
    RP_NEED_F3_STATE(b, d_jac);
    RP_HIP(rp::launch_solution_jacobian_vel(b->view, b->params, d_jac, b->stream));
    return RP_OK;
}

int rp_batch_bind_solution(rp_batch *b, rp_solution *d_out)
{
    if (!b) return fail(RP_ERR_INVALID, "null batch handle");
    if (((uintptr_t)d_out & 31u) != 0) return fail(RP_ERR_INVALID, "solution records must be 32-byte aligned");
    b->view.solution = reinterpret_cast<rp::Solution *>(d_out);
    solution_bound(b);      // the next gated launch that skips finished problems seeds it first
    return RP_OK;
}

int rp_batch_reduce_device(rp_batch *b, double *d_out4)
{
    RP_NEED_STATE(b);
    if (!d_out4) return fail(RP_ERR_INVALID, "null output");
    RP_HIP(rp::launch_reduce(b->view, b->params, b->ungated_steps * (double)b->view.n, b->d_scratch, d_out4, b->stream));
    return RP_OK;
}

int rp_batch_reduce(rp_batch *b, rp_reduction *out)
{
    RP_NEED(b);
    if (!out) return fail(RP_ERR_INVALID, "null output");
    const int st = rp_batch_reduce_device(b, b->d_scratch + 4096);
    return st == RP_OK ? read_summary(b, out) : st;
}

int rp_batch_summary_device(rp_batch *b, double **d_out4)
{
    RP_NEED(b);
    if (!d_out4) return fail(RP_ERR_INVALID, "null output");
    int st = rp_batch_reduce_device(b, b->d_scratch + 4096);
    if (st != RP_OK) return st;
    *d_out4 = b->d_scratch + 4096;
    return RP_OK;
}

int rp_batch_summary_read(rp_batch *b, rp_reduction *out)
{
    RP_NEED(b);
    if (!out) return fail(RP_ERR_INVALID, "null output");
    return read_summary(b, out);
}

int rp_batch_sample(rp_batch *b, double *pos66, double *acc4)
{
    RP_NEED_STATE(b);
    if (!pos66 || !acc4) return fail(RP_ERR_INVALID, "null output");
    const size_t n = b->view.n;
    double *d = nullptr;
    RP_HIP(hipMalloc((void **)&d, n * 70 * sizeof(double)));
    hipError_t e = rp::launch_sample(b->view, d, d + n * 66, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(pos66, d, n * 66 * sizeof(double), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(acc4, d + n * 66, n * 4 * sizeof(double), hipMemcpyDeviceToHost, b->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(RP_ERR_DEVICE, "rp_batch_sample: %s", hipGetErrorString(e));
    return RP_OK;
}

int rp_batch_sample_device(rp_batch *b, double *d_pos66, double *d_acc4)
{
    RP_NEED_STATE(b);
    if (!d_pos66 || !d_acc4) return fail(RP_ERR_INVALID, "null output");
    if (((uintptr_t)d_pos66 & 15u) != 0) return fail(RP_ERR_INVALID, "d_pos66 must be 16-byte aligned (the positions are written as 16-byte vectors)");
    if (samples_through_records(b)) {
        // a whole scheduled batch whose positions are still the ones it was given: through problem-order records (two coalesced
        // sectors per problem) instead of the per-field gather; same arithmetic, same bits
        if (!b->d_solscratch) RP_HIP(hipMalloc((void **)&b->d_solscratch, b->view.n * sizeof(rp::Solution)));
        b->view.iters_add = (int)b->ungated_steps;
        RP_HIP(rp::launch_sample_from_records(b->view, b->d_solscratch, d_pos66, d_acc4, b->stream));
        return RP_OK;
    }
    RP_HIP(rp::launch_sample(b->view, d_pos66, d_acc4, b->stream));
    return RP_OK;
}

// ---- what can be asked of a spline: its value at the caller's own times, the first crossing of a level, the extremes and the integrals
// over a window, and their derivatives (trajectory.hip; DESIGN.md sections 13-19) ----
namespace {

bool misaligned16(const void *p) { return ((uintptr_t)p & 15u) != 0; }

// all-null tables, for a table the caller left out
const double *const kNoInputs[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
double *const kNoOutputs[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};

bool any_of(double *const t[], int count)
{
    bool any = false;
    for (int f = 0; f < count; ++f) any = any || t[f];
    return any;
}

// What every one of these entries checks of its queries before any device call: the sizes; the one n x k array the entry cannot do
// without (`required`, under its name; the windowed entries have none: a null window end is -inf or +inf); the 16-byte alignment of
// every other n x k array that is read or written (null: not given); and that an output was asked for -- after the alignment where
// there is a required array, before it where there is none.
int check_queries(const char *who, size_t n, size_t k, const double *required, const char *name, std::initializer_list<const void *> per_query,
                  bool any_output)
{
    if (n == 0 || k == 0) return fail(RP_ERR_INVALID, "%s: n and k must be positive", who);
    if (k >= ((size_t)1 << 31)) return fail(RP_ERR_INVALID, "%s: k must be below 2^31", who);
    if (n > SIZE_MAX / sizeof(double) / k) return fail(RP_ERR_INVALID, "%s: n x k does not fit", who);
    if (name) {
        if (!required) return fail(RP_ERR_INVALID, "%s: %s is null", who, name);
        if (misaligned16(required)) return fail(RP_ERR_INVALID, "%s: %s must be 16-byte aligned (the queries move as 16-byte vectors)", who, name);
    } else if (!any_output) {
        return fail(RP_ERR_INVALID, "%s: no output asked for", who);
    }
    for (const void *array : per_query)
        if (misaligned16(array)) return fail(RP_ERR_INVALID, "%s: every n x k array must be 16-byte aligned (the queries move as 16-byte vectors)", who);
    if (!any_output) return fail(RP_ERR_INVALID, "%s: no output asked for", who);
    return RP_OK;
}

// a table of eight spline pointers, under the name the entry gives it
int check_spline(const char *who, const char *table, const double *const d_spline[8])
{
    if (!d_spline) return fail(RP_ERR_INVALID, "%s: %s is null", who, table);
    for (int f = 0; f < 8; ++f)
        if (!d_spline[f] && f != 3 && f != 4) return fail(RP_ERR_INVALID, "%s: %s[%d] is null (only the end velocities, [3] and [4], may be)", who, table, f);
    return RP_OK;
}

// the stateless entries: the device and the spline first
int check_stateless(const char *who, int device, const double *const d_spline[8], size_t n, size_t k, const double *required, const char *name,
                    std::initializer_list<const void *> per_query, bool any_output)
{
    if (device < 0) return fail(RP_ERR_INVALID, "%s: device %d", who, device);
    const int st = check_spline(who, "d_spline", d_spline);
    return st != RP_OK ? st : check_queries(who, n, k, required, name, per_query, any_output);
}

}  // namespace

int rp_trajectory_eval(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_tau, double *d_pos,
                       double *d_vel, double *d_acc)
{
    const int st = check_stateless(__func__, device, d_spline, n, k, d_tau, "d_tau", {d_pos, d_vel, d_acc}, d_pos || d_vel || d_acc);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_trajectory_eval(n, k, d_spline, d_tau, d_pos, d_vel, d_acc, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_eval_vjp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_tau,
                           const double *d_g_pos, const double *d_g_vel, const double *d_g_acc, double *const d_spline_bar[8], double *d_tau_bar)
{
    double *const *bars = d_spline_bar ? d_spline_bar : kNoOutputs;
    const int st = check_stateless(__func__, device, d_spline, n, k, d_tau, "d_tau", {d_g_pos, d_g_vel, d_g_acc, d_tau_bar}, d_tau_bar || any_of(bars, 8));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_trajectory_vjp(n, k, d_spline, d_tau, d_g_pos, d_g_vel, d_g_acc, bars, d_tau_bar, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_eval_jvp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_tau,
                           const double *const d_spline_dot[8], const double *d_tau_dot, double *d_pos_dot, double *d_vel_dot, double *d_acc_dot)
{
    const int st = check_stateless(__func__, device, d_spline, n, k, d_tau, "d_tau", {d_tau_dot, d_pos_dot, d_vel_dot, d_acc_dot},
                                   d_pos_dot || d_vel_dot || d_acc_dot);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_trajectory_jvp(n, k, d_spline, d_tau, d_spline_dot ? d_spline_dot : kNoInputs, d_tau_dot, d_pos_dot, d_vel_dot, d_acc_dot,
                                     (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_eval_hvp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_tau,
                           const double *d_g_pos, const double *d_g_vel, const double *d_g_acc, const double *const d_spline_dot[8],
                           const double *d_tau_dot, double *const d_spline_bar_dot[8], double *d_tau_bar_dot)
{
    double *const *bars = d_spline_bar_dot ? d_spline_bar_dot : kNoOutputs;
    const int st = check_stateless(__func__, device, d_spline, n, k, d_tau, "d_tau", {d_g_pos, d_g_vel, d_g_acc, d_tau_dot, d_tau_bar_dot},
                                   d_tau_bar_dot || any_of(bars, 8));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_trajectory_hvp(n, k, d_spline, d_tau, d_g_pos, d_g_vel, d_g_acc, d_spline_dot ? d_spline_dot : kNoInputs, d_tau_dot, bars,
                                     d_tau_bar_dot, (hipStream_t)stream));
    return RP_OK;
}

int rp_batch_trajectory_device(rp_batch *b, const double *d_tau, size_t k, double *d_pos, double *d_vel, double *d_acc)
{
    if (!b) return fail(RP_ERR_INVALID, "null batch handle");
    const int st = check_queries(__func__, b->view.n, k, d_tau, "d_tau", {d_pos, d_vel, d_acc}, d_pos || d_vel || d_acc);
    if (st != RP_OK) return st;
    RP_NEED_STATE(b);
    RP_HIP(rp::launch_trajectory_batch(b->view, d_tau, k, d_pos, d_vel, d_acc, b->stream));
    return RP_OK;
}

// the first time a spline reaches a level: the times are the output that cannot be left out
int rp_trajectory_crossing(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_level, double *d_time,
                           double *d_vel)
{
    const int st = check_stateless(__func__, device, d_spline, n, k, d_level, "d_level", {d_time, d_vel}, true);
    if (st != RP_OK) return st;
    if (!d_time) return fail(RP_ERR_INVALID, "%s: d_time is null", __func__);
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_crossing(n, k, d_spline, d_level, d_time, d_vel, (hipStream_t)stream));
    return RP_OK;
}

int rp_batch_crossing_device(rp_batch *b, const double *d_level, size_t k, double *d_time, double *d_vel)
{
    if (!b) return fail(RP_ERR_INVALID, "null batch handle");
    const int st = check_queries(__func__, b->view.n, k, d_level, "d_level", {d_time, d_vel}, true);
    if (st != RP_OK) return st;
    if (!d_time) return fail(RP_ERR_INVALID, "%s: d_time is null", __func__);
    RP_NEED_STATE(b);
    RP_HIP(rp::launch_crossing_batch(b->view, d_level, k, d_time, d_vel, b->stream));
    return RP_OK;
}

// the extreme position and velocity over a window: two tables of four outputs, which must hold at least one between them
int rp_trajectory_extrema(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi,
                          double *const d_value[4], double *const d_time[4])
{
    double *const *v = d_value ? d_value : kNoOutputs, *const *t = d_time ? d_time : kNoOutputs;
    const int st = check_stateless(__func__, device, d_spline, n, k, nullptr, nullptr, {d_lo, d_hi, v[0], v[1], v[2], v[3], t[0], t[1], t[2], t[3]},
                                   any_of(v, 4) || any_of(t, 4));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_extrema(n, k, d_spline, d_lo, d_hi, v, t, (hipStream_t)stream));
    return RP_OK;
}

int rp_batch_extrema_device(rp_batch *b, const double *d_lo, const double *d_hi, size_t k, double *const d_value[4], double *const d_time[4])
{
    if (!b) return fail(RP_ERR_INVALID, "null batch handle");
    double *const *v = d_value ? d_value : kNoOutputs, *const *t = d_time ? d_time : kNoOutputs;
    const int st = check_queries(__func__, b->view.n, k, nullptr, nullptr, {d_lo, d_hi, v[0], v[1], v[2], v[3], t[0], t[1], t[2], t[3]},
                                 any_of(v, 4) || any_of(t, 4));
    if (st != RP_OK) return st;
    RP_NEED_STATE(b);
    RP_HIP(rp::launch_extrema_batch(b->view, d_lo, d_hi, k, v, t, b->stream));
    return RP_OK;
}

// the extreme gap between two splines over a window: both spline tables, then the queries; two tables of two outputs
int rp_trajectory_gap(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8],
                      const double *d_lo, const double *d_hi, const double *d_delay, double *const d_value[2], double *const d_time[2])
{
    double *const *v = d_value ? d_value : kNoOutputs, *const *t = d_time ? d_time : kNoOutputs;
    if (device < 0) return fail(RP_ERR_INVALID, "%s: device %d", __func__, device);
    int st = check_spline(__func__, "d_spline_a", d_spline_a);
    if (st == RP_OK) st = check_spline(__func__, "d_spline_b", d_spline_b);
    if (st == RP_OK) st = check_queries(__func__, n, k, nullptr, nullptr, {d_lo, d_hi, d_delay, v[0], v[1], t[0], t[1]}, any_of(v, 2) || any_of(t, 2));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_gap(n, k, d_spline_a, d_spline_b, d_lo, d_hi, d_delay, v, t, (hipStream_t)stream));
    return RP_OK;
}

// the tracking integrals between two splines over a window and their first derivatives: rp_trajectory_gap's argument rules
static int check_tracking(const char *who, int device, const double *const d_spline_a[8], const double *const d_spline_b[8], size_t n, size_t k,
                          std::initializer_list<const void *> arrays, bool any_output)
{
    if (device < 0) return fail(RP_ERR_INVALID, "%s: device %d", who, device);
    int st = check_spline(who, "d_spline_a", d_spline_a);
    if (st == RP_OK) st = check_spline(who, "d_spline_b", d_spline_b);
    if (st == RP_OK) st = check_queries(who, n, k, nullptr, nullptr, arrays, any_output);
    return st;
}

int rp_trajectory_tracking(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8],
                           const double *d_lo, const double *d_hi, const double *d_delay, double *const d_value[3])
{
    double *const *v = d_value ? d_value : kNoOutputs;
    const int st = check_tracking(__func__, device, d_spline_a, d_spline_b, n, k, {d_lo, d_hi, d_delay, v[0], v[1], v[2]}, any_of(v, 3));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_tracking(n, k, d_spline_a, d_spline_b, d_lo, d_hi, d_delay, v, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_tracking_vjp(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8],
                               const double *d_lo, const double *d_hi, const double *d_delay, const double *const d_g[3],
                               double *const d_spline_a_bar[8], double *const d_spline_b_bar[8], double *d_lo_bar, double *d_hi_bar,
                               double *d_delay_bar)
{
    const double *const *g = d_g ? d_g : kNoInputs;
    double *const *bars_a = d_spline_a_bar ? d_spline_a_bar : kNoOutputs, *const *bars_b = d_spline_b_bar ? d_spline_b_bar : kNoOutputs;
    const int st = check_tracking(__func__, device, d_spline_a, d_spline_b, n, k, {d_lo, d_hi, d_delay, g[0], g[1], g[2], d_lo_bar, d_hi_bar, d_delay_bar},
                                  d_lo_bar || d_hi_bar || d_delay_bar || any_of(bars_a, 8) || any_of(bars_b, 8));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_tracking_vjp(n, k, d_spline_a, d_spline_b, d_lo, d_hi, d_delay, g, bars_a, bars_b, d_lo_bar, d_hi_bar, d_delay_bar,
                                   (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_tracking_jvp(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8],
                               const double *d_lo, const double *d_hi, const double *d_delay, const double *const d_spline_a_dot[8],
                               const double *const d_spline_b_dot[8], const double *d_lo_dot, const double *d_hi_dot, const double *d_delay_dot,
                               double *const d_value_dot[3])
{
    double *const *out = d_value_dot ? d_value_dot : kNoOutputs;
    const int st = check_tracking(__func__, device, d_spline_a, d_spline_b, n, k,
                                  {d_lo, d_hi, d_delay, d_lo_dot, d_hi_dot, d_delay_dot, out[0], out[1], out[2]}, any_of(out, 3));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_tracking_jvp(n, k, d_spline_a, d_spline_b, d_lo, d_hi, d_delay, d_spline_a_dot ? d_spline_a_dot : kNoInputs,
                                   d_spline_b_dot ? d_spline_b_dot : kNoInputs, d_lo_dot, d_hi_dot, d_delay_dot, out, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_tracking_hvp(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8],
                               const double *d_lo, const double *d_hi, const double *d_delay, const double *const d_g[3],
                               const double *const d_spline_a_dot[8], const double *const d_spline_b_dot[8], const double *d_lo_dot,
                               const double *d_hi_dot, const double *d_delay_dot, double *const d_spline_a_bar_dot[8],
                               double *const d_spline_b_bar_dot[8], double *d_lo_bar_dot, double *d_hi_bar_dot, double *d_delay_bar_dot)
{
    const double *const *g = d_g ? d_g : kNoInputs;
    double *const *bars_a = d_spline_a_bar_dot ? d_spline_a_bar_dot : kNoOutputs, *const *bars_b = d_spline_b_bar_dot ? d_spline_b_bar_dot : kNoOutputs;
    const int st = check_tracking(__func__, device, d_spline_a, d_spline_b, n, k,
                                  {d_lo, d_hi, d_delay, g[0], g[1], g[2], d_lo_dot, d_hi_dot, d_delay_dot, d_lo_bar_dot, d_hi_bar_dot, d_delay_bar_dot},
                                  d_lo_bar_dot || d_hi_bar_dot || d_delay_bar_dot || any_of(bars_a, 8) || any_of(bars_b, 8));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_tracking_hvp(n, k, d_spline_a, d_spline_b, d_lo, d_hi, d_delay, g, d_spline_a_dot ? d_spline_a_dot : kNoInputs,
                                   d_spline_b_dot ? d_spline_b_dot : kNoInputs, d_lo_dot, d_hi_dot, d_delay_dot, bars_a, bars_b, d_lo_bar_dot,
                                   d_hi_bar_dot, d_delay_bar_dot, (hipStream_t)stream));
    return RP_OK;
}

// the first time the gap between two splines reaches a level: rp_trajectory_gap's argument rules; the times cannot be left out
int rp_trajectory_meeting(int device, void *stream, size_t n, size_t k, const double *const d_spline_a[8], const double *const d_spline_b[8],
                          const double *d_level, const double *d_lo, const double *d_hi, const double *d_delay, double *d_time, double *d_relvel)
{
    const int st = check_tracking(__func__, device, d_spline_a, d_spline_b, n, k, {d_level, d_lo, d_hi, d_delay, d_time, d_relvel}, true);
    if (st != RP_OK) return st;
    if (!d_time) return fail(RP_ERR_INVALID, "%s: d_time is null", __func__);
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_meeting(n, k, d_spline_a, d_spline_b, d_level, d_lo, d_hi, d_delay, d_time, d_relvel, (hipStream_t)stream));
    return RP_OK;
}

// What the two pair entries in d axes check first: the device, d, and the two tables of 8 d pointers, axis-major (A's before B's per axis).
static int check_vehicles(const char *who, int device, int d, const double *const *d_spline_a, const double *const *d_spline_b)
{
    if (device < 0) return fail(RP_ERR_INVALID, "%s: device %d", who, device);
    if (d < 1 || d > 3) return fail(RP_ERR_INVALID, "%s: d must be 1, 2 or 3, got %d", who, d);
    if (!d_spline_a) return fail(RP_ERR_INVALID, "%s: d_spline_a is null", who);
    if (!d_spline_b) return fail(RP_ERR_INVALID, "%s: d_spline_b is null", who);
    int st = RP_OK;
    for (int x = 0; x < d && st == RP_OK; ++x) {
        st = check_spline(who, "d_spline_a", d_spline_a + 8 * x);
        if (st == RP_OK) st = check_spline(who, "d_spline_b", d_spline_b + 8 * x);
    }
    return st;
}

struct Required {
    const char *name;
    const void *given;
};

// What the four fleet entries check, in this order: the device, m, d, level_per_pair (null: the entry has none), the table of 8 d pointers,
// the entry's own required arrays under their names, that n x pairs fits, and check_queries of the n x pairs x k arrays.
static int check_fleet(const char *who, int device, size_t n, size_t m, size_t k, int d, const int *level_per_pair, const double *const *d_fleet,
                       std::initializer_list<Required> required, std::initializer_list<const void *> per_query, bool any_output)
{
    if (device < 0) return fail(RP_ERR_INVALID, "%s: device %d", who, device);
    if (m < 2 || m > 256) return fail(RP_ERR_INVALID, "%s: m must be 2..256 vehicles per scene, got %zu", who, m);
    if (d < 1 || d > 3) return fail(RP_ERR_INVALID, "%s: d must be 1, 2 or 3, got %d", who, d);
    if (level_per_pair && *level_per_pair != 0 && *level_per_pair != 1)
        return fail(RP_ERR_INVALID, "%s: level_per_pair must be 0 (n x k) or 1 (n x pairs x k), got %d", who, *level_per_pair);
    if (!d_fleet) return fail(RP_ERR_INVALID, "%s: d_fleet is null", who);
    for (int x = 0; x < d; ++x) {
        const int st = check_spline(who, "d_fleet", d_fleet + 8 * x);
        if (st != RP_OK) return st;
    }
    for (const Required &r : required)
        if (!r.given) return fail(RP_ERR_INVALID, "%s: %s is null", who, r.name);
    const size_t pairs = m * (m - 1) / 2;
    if (n > SIZE_MAX / sizeof(double) / pairs) return fail(RP_ERR_INVALID, "%s: n x pairs does not fit", who);
    return check_queries(who, n == 0 ? 0 : n * pairs, k, nullptr, nullptr, per_query, any_output);
}

// the least squared distance of two vehicles moving in d axes: two tables of 8 d pointers, axis-major; rp_trajectory_gap's argument rules
int rp_trajectory_separation(int device, void *stream, size_t n, size_t k, int d, const double *const *d_spline_a, const double *const *d_spline_b,
                             const double *d_lo, const double *d_hi, const double *d_delay, double *d_value, double *d_time)
{
    int st = check_vehicles(__func__, device, d, d_spline_a, d_spline_b);
    if (st == RP_OK) st = check_queries(__func__, n, k, nullptr, nullptr, {d_lo, d_hi, d_delay, d_value, d_time}, d_value || d_time);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_separation(n, k, d, d_spline_a, d_spline_b, d_lo, d_hi, d_delay, d_value, d_time, (hipStream_t)stream));
    return RP_OK;
}

// that least squared distance for every pair of n scenes of m vehicles: one table of 8 d pointers to n m values each; the windows are n x k
// and read as single values, the outputs n x pairs x k and written as 16-byte vectors
int rp_trajectory_fleet_separation(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_lo,
                                   const double *d_hi, double *d_value, double *d_time)
{
    const int st = check_fleet(__func__, device, n, m, k, d, nullptr, d_fleet, {}, {d_value, d_time}, d_value || d_time);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_fleet_separation(n, m, k, d, d_fleet, d_lo, d_hi, d_value, d_time, (hipStream_t)stream));
    return RP_OK;
}

// the first time that squared distance reaches a level: rp_trajectory_separation's tables and argument rules, a level and a time that are required
int rp_trajectory_contact(int device, void *stream, size_t n, size_t k, int d, const double *const *d_spline_a, const double *const *d_spline_b,
                          const double *d_level_sq, const double *d_lo, const double *d_hi, const double *d_delay, double *d_time, double *d_rate)
{
    int st = check_vehicles(__func__, device, d, d_spline_a, d_spline_b);
    if (st == RP_OK && !d_time) st = fail(RP_ERR_INVALID, "%s: d_time is null", __func__);
    if (st == RP_OK) st = check_queries(__func__, n, k, d_level_sq, "d_level_sq", {d_lo, d_hi, d_delay, d_time, d_rate}, true);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_contact(n, k, d, d_spline_a, d_spline_b, d_level_sq, d_lo, d_hi, d_delay, d_time, d_rate, (hipStream_t)stream));
    return RP_OK;
}

// that first time for every pair of n scenes of m vehicles: rp_trajectory_fleet_separation's table and windows; the level n x k and read as
// single values (level_per_pair 0) or n x pairs x k and read as 16-byte vectors (1); the outputs n x pairs x k
int rp_trajectory_fleet_contact(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_level_sq,
                                int level_per_pair, const double *d_lo, const double *d_hi, double *d_time, double *d_rate)
{
    const int st = check_fleet(__func__, device, n, m, k, d, &level_per_pair, d_fleet, {{"d_level_sq", d_level_sq}, {"d_time", d_time}},
                               {level_per_pair ? d_level_sq : nullptr, d_time, d_rate}, true);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_fleet_contact(n, m, k, d, d_fleet, d_level_sq, level_per_pair, d_lo, d_hi, d_time, d_rate, (hipStream_t)stream));
    return RP_OK;
}

// What the two cross entries check, in check_fleet's order: the device, m_a and m_b, d, level_per_pair (null: the entry has none), the two
// tables of 8 d pointers, the entry's own required arrays, that n x pairs fits, and check_queries of the n x pairs x k arrays.
static int check_cross(const char *who, int device, size_t n, size_t m_a, size_t m_b, size_t k, int d, const int *level_per_pair,
                       const double *const *d_fleet_a, const double *const *d_fleet_b, std::initializer_list<Required> required,
                       std::initializer_list<const void *> per_query, bool any_output)
{
    if (device < 0) return fail(RP_ERR_INVALID, "%s: device %d", who, device);
    if (m_a < 1 || m_a > 32768 || m_b < 1 || m_b > 32768)
        return fail(RP_ERR_INVALID, "%s: m_a and m_b must be 1..32768 vehicles per scene, got %zu and %zu", who, m_a, m_b);
    if (d < 1 || d > 3) return fail(RP_ERR_INVALID, "%s: d must be 1, 2 or 3, got %d", who, d);
    if (level_per_pair && *level_per_pair != 0 && *level_per_pair != 1)
        return fail(RP_ERR_INVALID, "%s: level_per_pair must be 0 (n x k) or 1 (n x pairs x k), got %d", who, *level_per_pair);
    if (!d_fleet_a) return fail(RP_ERR_INVALID, "%s: d_fleet_a is null", who);
    if (!d_fleet_b) return fail(RP_ERR_INVALID, "%s: d_fleet_b is null", who);
    for (int x = 0; x < d; ++x) {
        int st = check_spline(who, "d_fleet_a", d_fleet_a + 8 * x);
        if (st == RP_OK) st = check_spline(who, "d_fleet_b", d_fleet_b + 8 * x);
        if (st != RP_OK) return st;
    }
    for (const Required &r : required)
        if (!r.given) return fail(RP_ERR_INVALID, "%s: %s is null", who, r.name);
    const size_t pairs = m_a * m_b;
    if (n > SIZE_MAX / sizeof(double) / pairs) return fail(RP_ERR_INVALID, "%s: n x pairs does not fit", who);
    return check_queries(who, n == 0 ? 0 : n * pairs, k, nullptr, nullptr, per_query, any_output);
}

// the two fleet queries for every vehicle of fleet A against every vehicle of fleet B: two tables of 8 d pointers, to
// n m_a and n m_b values each; windows, level layouts and outputs as in the fleet entries, the outputs n x m_a m_b x k
int rp_trajectory_cross_separation(int device, void *stream, size_t n, size_t m_a, size_t m_b, size_t k, int d, const double *const *d_fleet_a,
                                   const double *const *d_fleet_b, const double *d_lo, const double *d_hi, double *d_value, double *d_time)
{
    const int st = check_cross(__func__, device, n, m_a, m_b, k, d, nullptr, d_fleet_a, d_fleet_b, {}, {d_value, d_time}, d_value || d_time);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_cross_separation(n, m_a, m_b, k, d, d_fleet_a, d_fleet_b, d_lo, d_hi, d_value, d_time, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_cross_contact(int device, void *stream, size_t n, size_t m_a, size_t m_b, size_t k, int d, const double *const *d_fleet_a,
                                const double *const *d_fleet_b, const double *d_level_sq, int level_per_pair, const double *d_lo,
                                const double *d_hi, double *d_time, double *d_rate)
{
    const int st = check_cross(__func__, device, n, m_a, m_b, k, d, &level_per_pair, d_fleet_a, d_fleet_b,
                               {{"d_level_sq", d_level_sq}, {"d_time", d_time}}, {level_per_pair ? d_level_sq : nullptr, d_time, d_rate}, true);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_cross_contact(n, m_a, m_b, k, d, d_fleet_a, d_fleet_b, d_level_sq, level_per_pair, d_lo, d_hi, d_time, d_rate,
                                    (hipStream_t)stream));
    return RP_OK;
}

// the two fleet entries with a start time per vehicle (n x m, read as single values): the refusals of the entries they extend, a start that is
// required, and three outputs of which any may be left out but not all
int rp_trajectory_fleet_separation_staggered(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                             const double *d_start, const double *d_lo, const double *d_hi, double *d_value, double *d_time,
                                             double *d_time_local)
{
    const int st = check_fleet(__func__, device, n, m, k, d, nullptr, d_fleet, {{"d_start", d_start}}, {d_value, d_time, d_time_local},
                               d_value || d_time || d_time_local);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_fleet_separation_staggered(n, m, k, d, d_fleet, d_start, d_lo, d_hi, d_value, d_time, d_time_local, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_fleet_contact_staggered(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                          const double *d_start, const double *d_level_sq, int level_per_pair, const double *d_lo,
                                          const double *d_hi, double *d_time, double *d_time_local, double *d_rate)
{
    const int st = check_fleet(__func__, device, n, m, k, d, &level_per_pair, d_fleet, {{"d_start", d_start}, {"d_level_sq", d_level_sq}},
                               {level_per_pair ? d_level_sq : nullptr, d_time, d_time_local, d_rate}, d_time || d_time_local || d_rate);
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_fleet_contact_staggered(n, m, k, d, d_fleet, d_start, d_level_sq, level_per_pair, d_lo, d_hi, d_time, d_time_local, d_rate,
                                              (hipStream_t)stream));
    return RP_OK;
}

// the fleet's position boxes over the scenes' windows: two tables of d pointers to n x m x k, of which at least one
// array must be given; the fleet entries' first refusals, then the entry's own required arrays.  d_start given: the window of vehicle v on
// its own clock, [lo - start_v, hi - start_v] (section 31).
static int fleet_reach(const char *who, int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                       const double *d_start, std::initializer_list<Required> required, const double *d_lo, const double *d_hi,
                       double *const *d_min, double *const *d_max)
{
    if (device < 0) return fail(RP_ERR_INVALID, "%s: device %d", who, device);
    if (m < 2 || m > 256) return fail(RP_ERR_INVALID, "%s: m must be 2..256 vehicles per scene, got %zu", who, m);
    if (d < 1 || d > 3) return fail(RP_ERR_INVALID, "%s: d must be 1, 2 or 3, got %d", who, d);
    if (!d_fleet) return fail(RP_ERR_INVALID, "%s: d_fleet is null", who);
    for (int x = 0; x < d; ++x) {
        const int st = check_spline(who, "d_fleet", d_fleet + 8 * x);
        if (st != RP_OK) return st;
    }
    if (n > SIZE_MAX / sizeof(double) / m) return fail(RP_ERR_INVALID, "%s: n x m does not fit", who);
    bool any = false;
    for (int x = 0; x < d; ++x) any = any || (d_min && d_min[x]) || (d_max && d_max[x]);
    const int st = check_queries(who, n == 0 ? 0 : n * m, k, nullptr, nullptr, {}, any);      // (the windows are read as single values)
    if (st != RP_OK) return st;
    for (int x = 0; x < d; ++x)
        if ((d_min && misaligned16(d_min[x])) || (d_max && misaligned16(d_max[x])))
            return fail(RP_ERR_INVALID, "%s: every n x m x k array must be 16-byte aligned (the queries move as 16-byte vectors)", who);
    for (const Required &r : required)
        if (!r.given) return fail(RP_ERR_INVALID, "%s: %s is null", who, r.name);
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_fleet_reach(n, m, k, d, d_fleet, d_start, d_lo, d_hi, d_min, d_max, nullptr, nullptr, nullptr, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_fleet_reach(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet, const double *d_lo,
                              const double *d_hi, double *const *d_min, double *const *d_max)
{
    return fleet_reach(__func__, device, stream, n, m, k, d, d_fleet, nullptr, {}, d_lo, d_hi, d_min, d_max);
}

int rp_trajectory_fleet_reach_staggered(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                        const double *d_start, const double *d_lo, const double *d_hi, double *const *d_min,
                                        double *const *d_max)
{
    return fleet_reach(__func__, device, stream, n, m, k, d, d_fleet, d_start, {{"d_start", d_start}}, d_lo, d_hi, d_min, d_max);
}

static int cull_workspace_size(const char *who, size_t n, size_t m, size_t k, int d, size_t *bytes, bool staggered)
{
    if (!bytes) return fail(RP_ERR_INVALID, "%s: bytes is null", who);
    *bytes = 0;
    if (m < 2 || m > 256) return fail(RP_ERR_INVALID, "%s: m must be 2..256 vehicles per scene, got %zu", who, m);
    if (d < 1 || d > 3) return fail(RP_ERR_INVALID, "%s: d must be 1, 2 or 3, got %d", who, d);
    if (n == 0 || k == 0) return fail(RP_ERR_INVALID, "%s: n and k must be positive", who);
    if (k >= ((size_t)1 << 31)) return fail(RP_ERR_INVALID, "%s: k must be below 2^31", who);
    const size_t need = rp::fleet_cull_workspace_bytes(n, m, k, d, staggered);
    if (need == 0) return fail(RP_ERR_INVALID, "%s: n x pairs must be below 2^32 and the boxes must fit", who);
    *bytes = need;
    return RP_OK;
}

int rp_trajectory_fleet_contact_culled_workspace(size_t n, size_t m, size_t k, int d, size_t *bytes)
{
    return cull_workspace_size(__func__, n, m, k, d, bytes, false);
}

int rp_trajectory_fleet_contact_staggered_culled_workspace(size_t n, size_t m, size_t k, int d, size_t *bytes)
{
    return cull_workspace_size(__func__, n, m, k, d, bytes, true);
}

// The culled and the candidates entries (DESIGN.md sections 30 to 32): the refusals of rp_trajectory_fleet_contact (d_start null) or
// rp_trajectory_fleet_contact_staggered in their order, with the entry's own required arrays; then n x pairs below 2^32 (a list entry is 32
// bits) and a workspace that is given, 16-byte aligned and large enough.  All three outputs null: the broad phase alone.
static int fleet_culled(const char *who, int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                        const double *d_start, const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi,
                        std::initializer_list<Required> required, double *d_time, double *d_time_local, double *d_rate, bool any_output,
                        void *d_workspace, size_t workspace_bytes, unsigned char *d_kept, uint32_t *d_list, uint32_t *d_count)
{
    const int st = check_fleet(who, device, n, m, k, d, &level_per_pair, d_fleet, required,
                               {level_per_pair ? d_level_sq : nullptr, d_time, d_time_local, d_rate}, any_output);
    if (st != RP_OK) return st;
    const bool staggered = d_start != nullptr;      // (an entry with starts has them among its required arrays)
    const size_t need = rp::fleet_cull_workspace_bytes(n, m, k, d, staggered);
    if (need == 0) return fail(RP_ERR_INVALID, "%s: n x pairs must be below 2^32 and the boxes must fit", who);
    if (!d_workspace) return fail(RP_ERR_INVALID, "%s: d_workspace is null", who);
    if (misaligned16(d_workspace)) return fail(RP_ERR_INVALID, "%s: d_workspace must be 16-byte aligned", who);
    if (workspace_bytes < need)
        return fail(RP_ERR_INVALID, "%s: the workspace holds %zu bytes, rp_trajectory_fleet_contact_%sculled_workspace asks for %zu", who,
                    workspace_bytes, staggered ? "staggered_" : "", need);
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_fleet_contact_culled(n, m, k, d, d_fleet, d_start, d_level_sq, level_per_pair, d_lo, d_hi, d_time, d_time_local, d_rate,
                                           d_workspace, d_kept, d_list, d_count, (hipStream_t)stream));
    return RP_OK;
}

// rp_trajectory_fleet_contact with the broad phase in front
int rp_trajectory_fleet_contact_culled(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                       const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi, double *d_time,
                                       double *d_rate, void *d_workspace, size_t workspace_bytes, unsigned char *d_kept, uint32_t *d_list,
                                       uint32_t *d_count)
{
    return fleet_culled(__func__, device, stream, n, m, k, d, d_fleet, nullptr, d_level_sq, level_per_pair, d_lo, d_hi,
                        {{"d_level_sq", d_level_sq}, {"d_time", d_time}}, d_time, nullptr, d_rate, true, d_workspace, workspace_bytes, d_kept,
                        d_list, d_count);
}

// the broad phase alone: the keep-flags of rp_trajectory_fleet_contact_culled's sieve, and no search
int rp_trajectory_fleet_contact_candidates(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                           const double *d_level_sq, int level_per_pair, const double *d_lo, const double *d_hi,
                                           void *d_workspace, size_t workspace_bytes, unsigned char *d_kept)
{
    return fleet_culled(__func__, device, stream, n, m, k, d, d_fleet, nullptr, d_level_sq, level_per_pair, d_lo, d_hi,
                        {{"d_level_sq", d_level_sq}, {"d_kept", d_kept}}, nullptr, nullptr, nullptr, true, d_workspace, workspace_bytes, d_kept,
                        nullptr, nullptr);
}

// rp_trajectory_fleet_contact_staggered with the broad phase in front
int rp_trajectory_fleet_contact_staggered_culled(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                                 const double *d_start, const double *d_level_sq, int level_per_pair, const double *d_lo,
                                                 const double *d_hi, double *d_time, double *d_time_local, double *d_rate, void *d_workspace,
                                                 size_t workspace_bytes, unsigned char *d_kept, uint32_t *d_list, uint32_t *d_count)
{
    return fleet_culled(__func__, device, stream, n, m, k, d, d_fleet, d_start, d_level_sq, level_per_pair, d_lo, d_hi,
                        {{"d_start", d_start}, {"d_level_sq", d_level_sq}}, d_time, d_time_local, d_rate, d_time || d_time_local || d_rate,
                        d_workspace, workspace_bytes, d_kept, d_list, d_count);
}

// its broad phase alone: the keep-flags, and no search
int rp_trajectory_fleet_contact_staggered_candidates(int device, void *stream, size_t n, size_t m, size_t k, int d, const double *const *d_fleet,
                                                     const double *d_start, const double *d_level_sq, int level_per_pair, const double *d_lo,
                                                     const double *d_hi, void *d_workspace, size_t workspace_bytes, unsigned char *d_kept)
{
    return fleet_culled(__func__, device, stream, n, m, k, d, d_fleet, d_start, d_level_sq, level_per_pair, d_lo, d_hi,
                        {{"d_start", d_start}, {"d_level_sq", d_level_sq}, {"d_kept", d_kept}}, nullptr, nullptr, nullptr, true, d_workspace,
                        workspace_bytes, d_kept, nullptr, nullptr);
}

// the integrals over a window, their first derivatives and the reverse rule's derivative along a direction
int rp_trajectory_integrals(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi,
                            double *const d_value[4])
{
    double *const *v = d_value ? d_value : kNoOutputs;
    const int st = check_stateless(__func__, device, d_spline, n, k, nullptr, nullptr, {d_lo, d_hi, v[0], v[1], v[2], v[3]}, any_of(v, 4));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_integrals(n, k, d_spline, d_lo, d_hi, v, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_integrals_vjp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi,
                                const double *const d_g[4], double *const d_spline_bar[8], double *d_lo_bar, double *d_hi_bar)
{
    const double *const *g = d_g ? d_g : kNoInputs;
    double *const *bars = d_spline_bar ? d_spline_bar : kNoOutputs;
    const int st = check_stateless(__func__, device, d_spline, n, k, nullptr, nullptr, {d_lo, d_hi, g[0], g[1], g[2], g[3], d_lo_bar, d_hi_bar},
                                   d_lo_bar || d_hi_bar || any_of(bars, 8));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_integrals_vjp(n, k, d_spline, d_lo, d_hi, g, bars, d_lo_bar, d_hi_bar, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_integrals_jvp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi,
                                const double *const d_spline_dot[8], const double *d_lo_dot, const double *d_hi_dot, double *const d_value_dot[4])
{
    double *const *out = d_value_dot ? d_value_dot : kNoOutputs;
    const int st = check_stateless(__func__, device, d_spline, n, k, nullptr, nullptr, {d_lo, d_hi, d_lo_dot, d_hi_dot, out[0], out[1], out[2], out[3]},
                                   any_of(out, 4));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_integrals_jvp(n, k, d_spline, d_lo, d_hi, d_spline_dot ? d_spline_dot : kNoInputs, d_lo_dot, d_hi_dot, out, (hipStream_t)stream));
    return RP_OK;
}

int rp_trajectory_integrals_hvp(int device, void *stream, size_t n, size_t k, const double *const d_spline[8], const double *d_lo, const double *d_hi,
                                const double *const d_g[4], const double *const d_spline_dot[8], const double *d_lo_dot, const double *d_hi_dot,
                                double *const d_spline_bar_dot[8], double *d_lo_bar_dot, double *d_hi_bar_dot)
{
    const double *const *g = d_g ? d_g : kNoInputs;
    double *const *bars = d_spline_bar_dot ? d_spline_bar_dot : kNoOutputs;
    const int st = check_stateless(__func__, device, d_spline, n, k, nullptr, nullptr,
                                   {d_lo, d_hi, g[0], g[1], g[2], g[3], d_lo_dot, d_hi_dot, d_lo_bar_dot, d_hi_bar_dot},
                                   d_lo_bar_dot || d_hi_bar_dot || any_of(bars, 8));
    if (st != RP_OK) return st;
    RP_HIP(hipSetDevice(device));
    RP_HIP(rp::launch_integrals_hvp(n, k, d_spline, d_lo, d_hi, g, d_spline_dot ? d_spline_dot : kNoInputs, d_lo_dot, d_hi_dot, bars, d_lo_bar_dot,
                                    d_hi_bar_dot, (hipStream_t)stream));
    return RP_OK;
}

int rp_batch_integrals_device(rp_batch *b, const double *d_lo, const double *d_hi, size_t k, double *const d_value[4])
{
    if (!b) return fail(RP_ERR_INVALID, "null batch handle");
    double *const *v = d_value ? d_value : kNoOutputs;
    const int st = check_queries(__func__, b->view.n, k, nullptr, nullptr, {d_lo, d_hi, v[0], v[1], v[2], v[3]}, any_of(v, 4));
    if (st != RP_OK) return st;
    RP_NEED_STATE(b);
    RP_HIP(rp::launch_integrals_batch(b->view, d_lo, d_hi, k, v, b->stream));
    return RP_OK;
}

int rp_batch_sample_range(rp_batch *b, size_t first, size_t count, double *pos66, double *acc4)
{
    RP_NEED_STATE(b);
    int st = check_range(b, first, count, pos66);
    if (st == RP_OK && !acc4) st = fail(RP_ERR_INVALID, "null output");
    if (st != RP_OK) return st;
    const size_t acc_at = kRangeChunk * 66;      // the staging buffer holds a chunk's positions, then its accelerations
    return read_range(b, first, count,
                      [&](size_t f, size_t c) { return rp::launch_sample_range(b->view, f, c, b->d_range, b->d_range + acc_at, b->stream); },
                      [&](size_t done, size_t c) {
                          const hipError_t e = hipMemcpyAsync(pos66 + done * 66, b->d_range, c * 66 * sizeof(double), hipMemcpyDeviceToHost, b->stream);
                          return e != hipSuccess ? e : hipMemcpyAsync(acc4 + done * 4, b->d_range + acc_at, c * 4 * sizeof(double), hipMemcpyDeviceToHost, b->stream);
                      });
}

int rp_batch_constraints_range(rp_batch *b, size_t first, size_t count, double *rows)
{
    RP_NEED_STATE(b);
    const int st = check_range(b, first, count, rows);
    if (st != RP_OK) return st;
    const size_t row = 1 + 14 * (size_t)rp::num_constraints(b->view.variant);
    return read_range(b, first, count,
                      [&](size_t f, size_t c) { return rp::launch_constraint_table(b->view, b->params, f, c, b->d_range, b->stream); },
                      [&](size_t done, size_t c) { return hipMemcpyAsync(rows + done * row, b->d_range, c * row * sizeof(double), hipMemcpyDeviceToHost, b->stream); });
}

int rp_batch_sync(rp_batch *b)
{
    RP_NEED(b);
    RP_HIP(hipStreamSynchronize(b->stream));
    return RP_OK;
}

int rp_batch_stream(rp_batch *b, void **stream)
{
    if (!b || !stream) return fail(RP_ERR_INVALID, "null argument");
    RP_NEED(b);      // the join: what the caller enqueues on the handle follows every solve enqueued so far
    *stream = (void *)b->stream;
    return RP_OK;
}

int rp_solve_overlap_set(int mode)
{
    if (mode < 0 || mode > 2) return fail(RP_ERR_INVALID, "overlap mode %d (want 0 = off, 1 = automatic, 2 = every eligible solve)", mode);
    g_overlap_mode.store(mode, std::memory_order_relaxed);
    return RP_OK;
}

int rp_solve_overlap_stats(unsigned long long out[4])
{
    if (!out) return fail(RP_ERR_INVALID, "null output");
    for (int i = 0; i < 4; ++i) out[i] = g_overlap_stats[i].load(std::memory_order_relaxed);
    return RP_OK;
}

int rp_batch_event_record(rp_batch *b, int slot)
{
    RP_NEED(b);
    if (slot < 0 || slot >= 8) return fail(RP_ERR_INVALID, "event slot %d out of range", slot);
    if (!b->event_live[slot]) {
        RP_HIP(hipEventCreate(&b->events[slot]));
        b->event_live[slot] = true;
    }
    RP_HIP(hipEventRecord(b->events[slot], b->stream));
    return RP_OK;
}

int rp_batch_event_elapsed_ms(rp_batch *b, int slot_start, int slot_stop, float *ms)
{
    RP_NEED(b);
    if (!ms || slot_start < 0 || slot_start >= 8 || slot_stop < 0 || slot_stop >= 8 || !b->event_live[slot_start] || !b->event_live[slot_stop])
        return fail(RP_ERR_INVALID, "events not recorded");
    RP_HIP(hipEventSynchronize(b->events[slot_stop]));
    RP_HIP(hipEventElapsedTime(ms, b->events[slot_start], b->events[slot_stop]));
    return RP_OK;
}

int rp_batch_field_ptr(rp_batch *b, int field, void **d_ptr)
{
    if (!b || !d_ptr) return fail(RP_ERR_INVALID, "null argument");
    if (field < 0 || field >= rp::state_len(b->view.variant)) return fail(RP_ERR_INVALID, "field %d out of range", field);
    RP_NEED_STATE(b);      // the caller is about to look at (or write) raw state: it has to exist
    *d_ptr = (char *)b->view.base + (size_t)field * b->view.stride * rp::storage_size(b->view.dtype);
    raw_pointer_out(b, field);
    return RP_OK;
}

int rp_batch_slot_map(rp_batch *b, uint32_t *slot_of_problem)
{
    RP_NEED(b);
    if (!slot_of_problem) return fail(RP_ERR_INVALID, "null output");
    const size_t n = b->view.n;
    if (!b->view.scheduled) {
        for (size_t i = 0; i < n; ++i) slot_of_problem[i] = (uint32_t)i;
        return RP_OK;
    }
    RP_HIP(hipMemcpyAsync(slot_of_problem, b->view.slot_of, n * sizeof(uint32_t), hipMemcpyDeviceToHost, b->stream));
    RP_HIP(hipStreamSynchronize(b->stream));
    return RP_OK;
}

// ---- rp_pipeline: positions in -> solutions out, batch after batch, with the batches dealt onto several streams ----
// Nothing but the entry points above, in the order a caller would issue them by hand: what it adds is the arrangement -- `depth` batches
// of n problems, slot j bound to stream j % n_streams at creation, job i in slot i % depth -- under which the scheduling pass of job
// i + 1 (three small memory- and latency-bound kernels) and the head of its solve run while job i's solve, a vector-ALU-bound kernel on
// the other stream, is still draining: wave slots stand empty 18 % of a lone 1 Mi-problem launch at its two ends (profiles/r5_tuning.md).
}  // extern "C"

struct rp_pipeline {
    int device, depth, n_streams;
    size_t n;
    hipStream_t streams[4];
    rp_batch **slots;
    hipEvent_t *done;          // per slot: recorded behind the slot's last job
    hipEvent_t *consumed;      // per slot: recorded behind that job's scheduling pass (its position arrays have been read)
    hipEvent_t inputs_ready;   // scratch: recorded on the caller's stream in rp_pipeline_submit
    hipStream_t prep[4];       // prep_mode != 0: the streams the jobs' scheduling passes run on, job i on prep[i % n_prep] (its solve waits for it through `consumed`)
    int n_prep;
    int prep_mode;             // RP_PIPELINE_PREP_*
    int64_t *job_of;           // per slot: the job it last took (-1: none)
    int64_t next_job;
};

extern "C" {

int rp_pipeline_create(rp_pipeline **out, int variant, int dtype, size_t n, int device, int depth, int n_streams)
{
    if (!out) return fail(RP_ERR_INVALID, "out is null");
    *out = nullptr;
    if (n_streams < 1 || n_streams > 4) return fail(RP_ERR_INVALID, "n_streams %d (want 1..4)", n_streams);
    if (depth < n_streams || depth > 1024 || depth % n_streams != 0)
        return fail(RP_ERR_INVALID, "depth %d (want a multiple of n_streams = %d, at most 1024)", depth, n_streams);
    rp_pipeline *p = new (std::nothrow) rp_pipeline();
    if (!p) return fail(RP_ERR_NOMEM, "host allocation failed");
    std::memset(p, 0, sizeof *p);
    p->device = device; p->depth = depth; p->n_streams = n_streams; p->n = n;
    p->slots = new (std::nothrow) rp_batch *[depth]();
    p->done = new (std::nothrow) hipEvent_t[depth]();
    p->consumed = new (std::nothrow) hipEvent_t[depth]();
    p->job_of = new (std::nothrow) int64_t[depth]();
    if (!p->slots || !p->done || !p->consumed || !p->job_of) { rp_pipeline_destroy(p); return fail(RP_ERR_NOMEM, "host allocation failed"); }
    for (int j = 0; j < depth; ++j) p->job_of[j] = -1;
    overlap_retire_lanes(device);      // the pipeline's streams want the hardware queues that idle auxiliary streams hold
    int st = RP_OK;
    for (int j = 0; j < depth && st == RP_OK; ++j) {
        // the first batch of a stream creates it (a non-blocking stream of its own); the others of that stream share it
        st = rp_batch_create(&p->slots[j], variant, dtype, n, device, j < n_streams ? nullptr : (void *)p->streams[j % n_streams]);
        if (st == RP_OK && j < n_streams) p->streams[j] = p->slots[j]->stream;
        if (st == RP_OK) p->slots[j]->slim_schedule = n_streams > 1;      // beside a running solve only one-wave blocks get in (schedule.hip)
        if (st == RP_OK) p->slots[j]->pipelined = true;                   // the pipeline deals its batches onto streams itself: no auxiliary lane
        if (st == RP_OK && hipEventCreateWithFlags(&p->done[j], hipEventDisableTiming) != hipSuccess) st = fail(RP_ERR_DEVICE, "hipEventCreate failed");
        if (st == RP_OK && hipEventCreateWithFlags(&p->consumed[j], hipEventDisableTiming) != hipSuccess) st = fail(RP_ERR_DEVICE, "hipEventCreate failed");
    }
    if (st == RP_OK && hipEventCreateWithFlags(&p->inputs_ready, hipEventDisableTiming) != hipSuccess) st = fail(RP_ERR_DEVICE, "hipEventCreate failed");
    // (default arrangement: the scheduling pass on the job's own stream.  A stream of its own for it -- rp_pipeline_set_prep -- measured the
    // same to 1 % in a process that owns few streams and WORSE in one that owns many: the HIP runtime multiplexes streams onto a handful of
    // hardware queues, GPU_MAX_HW_QUEUES = 4 by default, and two streams that share a queue serialise: profiles/r6_tuning.md)
    if (st != RP_OK) {
        char keep[sizeof g_err];
        std::memcpy(keep, g_err, sizeof keep);
        rp_pipeline_destroy(p);
        std::memcpy(g_err, keep, sizeof keep);
        return st;
    }
    *out = p;
    return RP_OK;
}

int rp_pipeline_destroy(rp_pipeline *p)
{
    if (!p) return RP_OK;
    (void)hipSetDevice(p->device);
    if (p->slots) {
        // batches that share a stream must go before the batch that owns it (slot j < n_streams owns stream j)
        for (int j = p->depth - 1; j >= 0; --j) if (p->slots[j]) rp_batch_destroy(p->slots[j]);
    }
    for (int j = 0; j < p->depth; ++j) {
        if (p->done && p->done[j]) (void)hipEventDestroy(p->done[j]);
        if (p->consumed && p->consumed[j]) (void)hipEventDestroy(p->consumed[j]);
    }
    if (p->inputs_ready) (void)hipEventDestroy(p->inputs_ready);
    for (int j = 0; j < p->n_prep; ++j) { (void)hipStreamSynchronize(p->prep[j]); (void)hipStreamDestroy(p->prep[j]); }
    delete[] p->slots;
    delete[] p->done;
    delete[] p->consumed;
    delete[] p->job_of;
    delete p;
    return RP_OK;
}

int rp_pipeline_set_prep(rp_pipeline *p, int mode)
{
    if (!p) return fail(RP_ERR_INVALID, "null pipeline handle");
    const bool fat = (mode & RP_PIPELINE_PREP_FAT_KERNELS) != 0;      // A/B: the 256-thread form of the pass whatever the arrangement
    mode &= ~RP_PIPELINE_PREP_FAT_KERNELS;
    if (mode != RP_PIPELINE_PREP_INLINE && mode != RP_PIPELINE_PREP_STREAM && mode != RP_PIPELINE_PREP_PRIORITY)
        return fail(RP_ERR_INVALID, "prep mode %d (want 0 = on the job's stream, 1 = a stream of its own, 2 = ... with the highest priority)", mode);
    if (p->next_job != 0) return fail(RP_ERR_INVALID, "the arrangement is fixed once a job has been submitted");
    RP_HIP(hipSetDevice(p->device));
    for (int j = 0; j < p->n_prep; ++j) (void)hipStreamDestroy(p->prep[j]);
    p->n_prep = 0;
    p->prep_mode = mode;
    for (int j = 0; j < p->depth; ++j) p->slots[j]->slim_schedule = !fat && (p->n_streams > 1 || mode != RP_PIPELINE_PREP_INLINE);
    if (mode == RP_PIPELINE_PREP_INLINE) return RP_OK;
    int least = 0, greatest = 0;
    if (mode == RP_PIPELINE_PREP_PRIORITY) RP_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
    // ONE prep stream: beside a running solve a pass takes about as long as the solve itself (three dependent, latency-bound kernels that
    // share every SIMD with four solve waves), which one stream just sustains; a prep stream per solve stream was measured and is no
    // faster -- two passes at once only contend (profiles/r6_pipeline_probe_two_prep_streams.log)
    RP_HIP(hipStreamCreateWithPriority(&p->prep[0], hipStreamNonBlocking, mode == RP_PIPELINE_PREP_PRIORITY ? greatest : 0));
    p->n_prep = 1;
    return RP_OK;
}

int rp_pipeline_set_params(rp_pipeline *p, const rp_params *params)
{
    if (!p || !params) return fail(RP_ERR_INVALID, "null argument");
    for (int j = 0; j < p->depth; ++j) {
        const int st = rp_batch_set_params(p->slots[j], params);
        if (st != RP_OK) return st;
    }
    return RP_OK;
}

int rp_pipeline_submit(rp_pipeline *p, const double *d_pos0, const double *d_pos1, const double *d_pos2, rp_solution *d_out,
                       double gap_tol, int max_iter, void *inputs_stream, int64_t *job)
{
    if (!p) return fail(RP_ERR_INVALID, "null pipeline handle");
    RP_HIP(hipSetDevice(p->device));
    const int64_t id = p->next_job;
    const int slot = (int)(id % p->depth);
    rp_batch *b = p->slots[slot];
    // The scheduling pass runs on the job's own stream or -- prep_mode -- on the pipeline's prep stream, behind the slot's previous job
    // (it overwrites the batch's order and records) and ahead of this job's solve (which waits for `consumed`).
    hipStream_t prep = p->n_prep ? p->prep[id % p->n_prep] : nullptr;
    hipStream_t solve_stream = b->stream, sched_stream = prep ? prep : b->stream;
    if (inputs_stream && (hipStream_t)inputs_stream != sched_stream) {      // the positions are produced by work on the caller's stream: wait for it, on the device
        RP_HIP(hipEventRecord(p->inputs_ready, (hipStream_t)inputs_stream));
        RP_HIP(hipStreamWaitEvent(sched_stream, p->inputs_ready, 0));
    }
    int st = rp_batch_bind_solution(b, d_out);
    if (st != RP_OK) return st;
    if (prep) {
        if (p->job_of[slot] >= 0) RP_HIP(hipStreamWaitEvent(prep, p->done[slot], 0));
        b->stream = prep;
        st = rp_batch_set_problems_device(b, d_pos0, d_pos1, d_pos2);
        b->stream = solve_stream;
    } else {
        st = rp_batch_set_problems_device(b, d_pos0, d_pos1, d_pos2);
    }
    if (st != RP_OK) return st;
    RP_HIP(hipEventRecord(p->consumed[slot], sched_stream));
    if (prep) RP_HIP(hipStreamWaitEvent(solve_stream, p->consumed[slot], 0));
    st = rp_batch_solve(b, gap_tol, max_iter, 0);
    if (st != RP_OK) return st;
    RP_HIP(hipEventRecord(p->done[slot], b->stream));
    p->job_of[slot] = id;
    p->next_job = id + 1;
    if (job) *job = id;
    return RP_OK;
}

static int pipeline_slot_of(rp_pipeline *p, int64_t job, int *slot)
{
    if (!p) return fail(RP_ERR_INVALID, "null pipeline handle");
    if (job < 0 || job >= p->next_job) return fail(RP_ERR_INVALID, "job %lld has not been submitted", (long long)job);
    *slot = (int)(job % p->depth);
    if (p->job_of[*slot] != job) return fail(RP_ERR_INVALID, "job %lld has left the pipeline: its slot holds job %lld", (long long)job, (long long)p->job_of[*slot]);
    return RP_OK;
}

int rp_pipeline_wait(rp_pipeline *p, int64_t job)
{
    if (!p) return fail(RP_ERR_INVALID, "null pipeline handle");
    RP_HIP(hipSetDevice(p->device));
    if (job < 0) {      // everything submitted so far
        for (int j = 0; j < p->n_prep; ++j) RP_HIP(hipStreamSynchronize(p->prep[j]));      // (first: a solve stream's last solve waits on them)
        for (int j = 0; j < p->n_streams; ++j) RP_HIP(hipStreamSynchronize(p->streams[j]));
        return RP_OK;
    }
    if (job >= p->next_job) return fail(RP_ERR_INVALID, "job %lld has not been submitted", (long long)job);
    const int slot = (int)(job % p->depth);
    RP_HIP(hipEventSynchronize(p->done[slot]));      // (the slot's LAST job: a later job of the same slot follows the asked one on one stream)
    return RP_OK;
}

int rp_pipeline_stream_wait(rp_pipeline *p, int64_t job, int what, void *stream)
{
    int slot = 0;
    const int st = pipeline_slot_of(p, job, &slot);
    if (st != RP_OK) return st;
    if (what != 0 && what != 1) return fail(RP_ERR_INVALID, "what = %d (0: the job's positions have been read, 1: its solutions are written)", what);
    RP_HIP(hipSetDevice(p->device));
    RP_HIP(hipStreamWaitEvent((hipStream_t)stream, what == 0 ? p->consumed[slot] : p->done[slot], 0));
    return RP_OK;
}

int rp_pipeline_batch(rp_pipeline *p, int64_t job, rp_batch **batch)
{
    if (!batch) return fail(RP_ERR_INVALID, "null output");
    int slot = 0;
    const int st = pipeline_slot_of(p, job, &slot);
    if (st != RP_OK) return st;
    *batch = p->slots[slot];
    return RP_OK;
}

}  // extern "C"
