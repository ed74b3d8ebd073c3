"""Torch layer over the batched F3 solve: tensors in, tensors out on the current stream, differentiable in the positions.

    vel1, duration0, duration1, iters, status = min_time_solve(pos0, pos1, pos2)
    (duration0 + duration1).sum().backward()      # -> pos0.grad, pos1.grad, pos2.grad
    vel1, duration0, duration1, iters, status, jac = min_time_jacobian(pos0, pos1, pos2)      # jac: (n, 3, 3)
    vel1, duration0, duration1, iters, status, jac, hess = min_time_hessian(pos0, pos1, pos2)      # hess: (n, 3, 3, 3)
    vel1, duration0, duration1, iters, status = min_time_solve(pos0, pos1, pos2, vel0=vel0, vel2=vel2)      # end velocities
    pos, vel, acc = trajectory_eval(pos0, pos1, pos2, vel1, duration0, duration1, tau)      # the spline at the caller's times, (n, k) each
    pos, vel, acc, vel1, duration0, duration1, iters, status = min_time_trajectory(pos0, pos1, pos2, tau)      # solve, then evaluate

The forward is Batch.set_problems_device + the fused gated solve + Batch.solution_device into a torch buffer, enqueued without
synchronising the host.  The backward is one rp_batch_solution_vjp launch at the state the forward left, the forward-mode rule
(torch.autograd.forward_ad, torch.func.jvp) one rp_batch_solution_jvp launch (include/rp_batch.h): the
implicit-function derivative of the central-path point the solve stopped at.  The backward is itself differentiable once more
(double backward: torch.autograd.grad(..., create_graph=True), torch.autograd.functional.hessian), through one
rp_batch_solution_jvp and one rp_batch_solution_hessian launch.  F3, float64 only; no vmap rule.

With end velocities (vel0= / vel2=) the forward is Batch.set_problems_vel_device instead, and the derivatives
in all five inputs come from rp_batch_solution_vjp_vel / rp_batch_solution_jvp_vel (first order only: a double backward raises
torch's once_differentiable error).  Without them the code path is the rest-to-rest one above, unchanged.

trajectory_eval is stateless: one rp_trajectory_eval launch on the current stream, differentiable to first order
in all eight spline inputs and in tau through one rp_trajectory_eval_vjp (backward) or rp_trajectory_eval_jvp (forward mode) launch.
min_time_trajectory composes it with min_time_solve, whose derivatives supply the rest of the chain.  With order=2 (section 17) the
evaluator's backward is differentiable once more: the backward of the backward is one rp_trajectory_eval_jvp launch (the part in the
upstream gradients) and one rp_trajectory_eval_hvp launch (the part in the spline inputs and tau); order=1, the default, is first order.
trajectory_crossing (section 14) is its inverse -- the first time the spline is at a level, one rp_trajectory_crossing launch -- with both
derivative modes composed from the evaluator's launches; min_time_crossing composes it with min_time_solve.
trajectory_extrema (section 15) answers how far and how fast at most: the extreme position and velocity over a window of times, one
rp_trajectory_extrema launch, both derivative modes one launch of the evaluator's at the times the extremes are attained, with the time's
own derivative routed to the window end or the duration the time is; min_time_extrema composes it with min_time_solve.
trajectory_integrals (section 16) answers how much: the integrals of pos, |vel|, vel^2 and acc^2 over a window of times, one
rp_trajectory_integrals launch, reverse mode one rp_trajectory_integrals_vjp launch, forward mode one rp_trajectory_integrals_jvp launch;
min_time_integrals composes it with min_time_solve; order=2 makes its backward differentiable once more (section 19): the backward of the
backward is one rp_trajectory_integrals_jvp launch and one rp_trajectory_integrals_hvp launch.
trajectory_gap (section 18) answers how close two splines in one frame get: the extreme of pos_a(t) - pos_b(t - delay) over a window of
times, one rp_trajectory_gap launch, both derivative modes one launch of the evaluator's on each spline at the times the extremes are
attained; min_time_gap composes it with two min_time_solve calls.
trajectory_tracking (section 20) answers how far apart they are on average: the integrals of that gap, of its square and of the square of
its rate over a window of times, one rp_trajectory_tracking launch, reverse mode one rp_trajectory_tracking_vjp call, forward mode one
rp_trajectory_tracking_jvp launch; min_time_tracking composes it with two min_time_solve calls; order=2 makes its backward differentiable
once more (section 23): the backward of the backward is one rp_trajectory_tracking_jvp launch and one rp_trajectory_tracking_hvp call.
trajectory_meeting (section 22) inverts that gap as trajectory_crossing inverts pos: the first time in a window at which the gap is at a
level, one rp_trajectory_meeting launch, both derivative modes one launch of the evaluator's on each spline through the implicit function
theorem; min_time_meeting composes it with two min_time_solve calls.
trajectory_separation (section 24) answers how close two vehicles that move in up to three axes get, each axis a spline of its own: the
least squared distance over a window of times and when it is attained, one rp_trajectory_separation launch, both derivative modes the
evaluator's launches on each axis' two splines at that time (the envelope theorem); synchronize_axes stretches a vehicle's axes to its
slowest; min_time_separation composes them with one min_time_solve call per vehicle over its axes.
trajectory_contact (section 25) inverts that squared distance as trajectory_meeting inverts the gap: the first time in a window at which the
two vehicles are within a radius, one rp_trajectory_contact launch, both derivative modes the evaluator's launches on each axis' two splines
through the implicit function theorem; min_time_contact composes it with the solves as min_time_separation does.
trajectory_fleet_separation (section 26) is trajectory_separation for every pair of a fleet, n scenes of m vehicles on one clock, in one
rp_trajectory_fleet_separation launch, bit for bit the pair call's; its derivatives are that call's routed per vehicle through a slot table
(fleet_slots), one evaluator launch and one derivative launch per axis on the n m splines, every sum a gather and a sum; fleet_pairs gives
the order of the pairs; min_time_fleet_separation composes it with one min_time_solve call over all axis problems.
trajectory_fleet_contact (section 27) is trajectory_contact for every pair of such a fleet in one rp_trajectory_fleet_contact launch, bit for
bit the pair call's, the level per scene or per pair; its derivatives are that call's implicit-function formula routed per vehicle through
the same slot table; min_time_fleet_contact composes it with the solves, and fleet_first_contact reduces the times to each scene's first
contact and the pair that makes it, in plain torch.
start= on those four (section 28) gives every vehicle a start time of its own on the scene's clock: pair (i, j) is the pair call with the
delay start_j - start_i over the window shifted by start_i, bit for bit, in one rp_trajectory_fleet_separation_staggered or
rp_trajectory_fleet_contact_staggered launch, differentiable in start through the same slot table; start=None is the call without it.
trajectory_cross_separation and trajectory_cross_contact (section 34) are the two pair calls for every vehicle of one fleet against every
vehicle of another, m_a m_b pairs row-major (cross_pairs), in one rp_trajectory_cross_separation or rp_trajectory_cross_contact launch, bit
for bit the pair call's; a vehicle of A owns a row of the output and a vehicle of B a column, so the derivatives are the fleet calls' with
a reshape or permute and a sum where those have the slot table; static_fleet makes the splines of obstacles that stand still;
min_time_cross_separation and min_time_cross_contact compose them with the solves.
"""
import collections
import ctypes
import functools
import threading

import torch

from . import capi
from .batch import Batch

_PARAM_FIELDS = {name for name, _ in capi.Params._fields_}


class _Pool:
    """Batches keyed by (device, n, stream): no hipMalloc / hipFree per call (hipFree synchronises the device).  A batch is out of
    the pool while an autograd graph may still call its backward; it comes back when that graph is freed."""

    def __init__(self):
        self._free = {}
        self._lock = threading.Lock()

    def take(self, key):
        with self._lock:
            free = self._free.get(key)
            if free:
                return free.pop()
        device, n, stream = key
        return Batch(n, capi.VARIANT_F3, capi.DTYPE_F64, device=device, stream=stream or None)

    def give(self, key, batch):
        with self._lock:
            self._free.setdefault(key, []).append(batch)

    def clear(self):
        with self._lock:
            batches = [b for free in self._free.values() for b in free]
            self._free.clear()
        for b in batches:
            b.close()


_pool = _Pool()


class _Lease:
    """The batch an autograd graph holds for its backward; returned to the pool when the graph (and with it this object) goes."""

    def __init__(self, key, batch):
        self.key, self.batch = key, batch

    def __del__(self):
        try:
            _pool.give(self.key, self.batch)
        except Exception:
            pass


def _stream_handle(stream):
    return stream.cuda_stream


def _check_is_tensor(name, t, who):
    if not isinstance(t, torch.Tensor):
        raise TypeError(who + ": %s must be a torch.Tensor, got %s" % (name, type(t).__name__))


def _check_is_float64(name, t, who):
    if t.dtype != torch.float64:
        raise TypeError(who + ": %s has dtype %s; float64 is required" % (name, t.dtype))


def _check_positions(pos0, pos1, pos2, who="min_time_solve"):
    for name, t in (("pos0", pos0), ("pos1", pos1), ("pos2", pos2)):
        _check_is_tensor(name, t, who)
        if t.device.type != "cuda":
            raise TypeError(who + ": %s is on %s; the solve runs on a ROCm device only (move it with .cuda())" % (name, t.device))
        _check_is_float64(name, t, who)
        if t.dim() != 1:
            raise ValueError(who + ": %s must be 1-D, got shape %s" % (name, tuple(t.shape)))
    if not (pos0.shape == pos1.shape == pos2.shape):
        raise ValueError(who + ": lengths differ (%d, %d, %d)" % (pos0.shape[0], pos1.shape[0], pos2.shape[0]))
    if not (pos0.device == pos1.device == pos2.device):
        raise ValueError(who + ": positions on different devices (%s, %s, %s)" % (pos0.device, pos1.device, pos2.device))
    if pos0.shape[0] == 0:
        raise ValueError(who + ": empty batch")


def _check_velocities(pos0, vel0, vel2, who):
    """Whether end velocities were given; each given one must be a 1-D float64 tensor on the positions' ROCm device, of their length."""
    if vel0 is None and vel2 is None:
        return False
    for name, t in (("vel0", vel0), ("vel2", vel2)):
        if t is None:
            continue
        _check_is_tensor(name, t, who)
        if t.device.type != "cuda" or t.device != pos0.device:
            raise TypeError(who + ": %s is on %s; it must be on the positions' ROCm device %s" % (name, t.device, pos0.device))
        _check_is_float64(name, t, who)
        if t.shape != pos0.shape:
            raise ValueError(who + ": %s has shape %s, the positions %s" % (name, tuple(t.shape), tuple(pos0.shape)))
    return True


def _check_params(params, who):
    if params is not None:
        unknown = set(params) - _PARAM_FIELDS
        if unknown:
            raise ValueError("%s: unknown rp_params field(s) %s" % (who, sorted(unknown)))


def _run_on(batch_stream, cur):
    """Context of a call whose work goes to the batch stream: the batch stream waits for `cur` before, `cur` for it after.  When
    the two are the same stream (any stream but the null stream), nothing is added."""
    class _Order:
        def __enter__(self):
            if batch_stream is not None:
                batch_stream.wait_stream(cur)

        def __exit__(self, *exc):
            if batch_stream is not None:
                cur.wait_stream(batch_stream)
    return _Order()


def _solve(pos0, pos1, pos2, gap_tol, max_iter, params, jacobian=False, hessian=False, vel=None):
    """Enqueue the solve on the current stream with a batch taken from the pool: (key, batch, (vel1, dur0, dur1, iters, status)),
    and the (n, 3, 3) Jacobian at the end when `jacobian`, the Jacobian and the (n, 3, 3, 3) Hessian (one launch) when `hessian`.
    vel = (vel0, vel2) (either may be None: zeros) poses the problems with end velocities: the Jacobian is then the (n, 3, 5) one in
    (pos0, pos1, pos2, vel0, vel2), the Hessian still the positions' (its own launch).  The caller gives the batch back or leases it."""
    device = pos0.device.index if pos0.device.index is not None else torch.cuda.current_device()
    n = pos0.shape[0]
    cur = torch.cuda.current_stream(device)
    handle = _stream_handle(cur)
    key = (device, n, handle)
    batch = _pool.take(key)
    # the null stream cannot be handed to a batch (NULL = "create your own"): then the batch's own stream is ordered by events
    ext = None if handle else torch.cuda.ExternalStream(batch.stream(), device=pos0.device)
    p0, p1, p2 = (t.contiguous() for t in (pos0, pos1, pos2))
    v0, v2 = (t.contiguous() if t is not None else None for t in (vel if vel is not None else (None, None)))
    out = torch.empty((n, 4), dtype=torch.float64, device=pos0.device)      # n rp_solution records (torch's blocks: 512-byte aligned)
    jac = torch.empty((n, 3, 5 if vel is not None else 3), dtype=torch.float64, device=pos0.device) if jacobian or hessian else None
    hess = torch.empty((n, 3, 3, 3), dtype=torch.float64, device=pos0.device) if hessian else None
    try:
        p = capi.Params()
        batch._lib.rp_params_default(ctypes.byref(p))
        for k, v in (params or {}).items():
            setattr(p, k, v)
        capi.check(batch._lib.rp_batch_set_params(batch._h, ctypes.byref(p)))
        with _run_on(ext, cur):
            if vel is None:
                batch.set_problems_device(p0.data_ptr(), p1.data_ptr(), p2.data_ptr())
            else:
                batch.set_problems_vel_device(p0.data_ptr(), p1.data_ptr(), p2.data_ptr(), *[t.data_ptr() if t is not None else 0 for t in (v0, v2)])
            batch.solve(gap_tol, max_iter, 0)
            batch.solution_device(out.data_ptr())
            if vel is not None:
                if hess is not None:
                    batch.solution_hessian(0, hess.data_ptr())
                if jac is not None:
                    batch.solution_jacobian_vel(jac.data_ptr())
            elif hess is not None:
                batch.solution_hessian(jac.data_ptr(), hess.data_ptr())
            elif jac is not None:
                batch.solution_jacobian(jac.data_ptr())
        if ext is not None:
            for t in (p0, p1, p2, v0, v2, out, jac, hess):
                if t is not None:
                    t.record_stream(ext)
    except Exception:
        _pool.give(key, batch)
        raise
    vel1, dur0, dur1 = out[:, 0].clone(), out[:, 1].clone(), out[:, 2].clone()
    words = out.view(torch.int32).view(n, 8)
    iters, status = words[:, 6].clone(), words[:, 7].clone()
    return key, batch, (vel1, dur0, dur1, iters, status) + tuple(t for t in (jac, hess) if t is not None)


def _plain(t):
    """The tensor under torch.func's wrappers: inside a transform the jvp rule receives its tangents, and creates its buffers, as
    wrapped tensors, which have no storage of their own; the kernel reads and writes the one they wrap."""
    while torch._C._functorch.is_functorch_wrapped_tensor(t):
        t = torch._C._functorch.get_unwrapped(t)
    return t


class _Holder:
    """How forward's batch reaches setup_context (in the setup_context form forward has no ctx): a non-tensor argument of apply."""
    __slots__ = ("lease",)

    def __init__(self):
        self.lease = None


def _launch(batch, device, launches, plain=False):
    """Enqueue derivative kernels at the state of `batch` from the current stream, as one ordered region: the batch stream waits
    for the current stream, runs them, and the current stream waits for it (_run_on; nothing is added when the two are the same
    stream), and every tensor the kernels touch is recorded on the batch stream.  launches: (bound Batch method, input tensors --
    None: a null address, which the kernels read as zeros --, number of outputs, their shape) each; the method gets the inputs'
    addresses, then the outputs'.  Returns one list of new float64 tensors per launch.  plain: the caller is a jvp rule, whose
    tensors the kernels read and write under torch.func's wrappers (_plain)."""
    cur = torch.cuda.current_stream(device)
    bstream = torch.cuda.ExternalStream(batch.stream(), device=device)
    same = bstream.cuda_stream == cur.cuda_stream
    unwrap = _plain if plain else (lambda t: t)
    jobs, results = [], []
    for method, inputs, count, shape in launches:
        ins = [unwrap(t.contiguous()) if t is not None else None for t in inputs]
        outs = [torch.empty(shape, dtype=torch.float64, device=device) for _ in range(count)]
        jobs.append((method, ins, [unwrap(t) for t in outs]))
        results.append(outs)
    with _run_on(None if same else bstream, cur):
        for method, ins, raw in jobs:
            method(*[t.data_ptr() if t is not None else 0 for t in ins], *[t.data_ptr() for t in raw])
    if not same:
        for _, ins, raw in jobs:
            for t in ins + raw:
                if t is not None:
                    t.record_stream(bstream)
    return results


def _forward(holder, *solve_args, **solve_kw):
    """forward of both solve Functions: the solve, its batch leased to the holder."""
    key, batch, outs = _solve(*solve_args, **solve_kw)
    holder.lease = _Lease(key, batch)
    return outs


def _setup_context(ctx, inputs, output):
    """setup_context of both solve Functions.  ctx keeps the lease, and with it the batch whose state backward and jvp differentiate,
    out of the pool: for as long as an autograd graph holds ctx, or only until apply returns when none does (no_grad, or no input
    requiring grad).  The holder goes when min_time_solve returns, so a batch nothing holds is back in the pool once its read-back
    is enqueued."""
    ctx.lease = inputs[-1].lease
    ctx.device = inputs[0].device
    ctx.mark_non_differentiable(output[3], output[4])


def _jvp(ctx, method, tangents):
    """jvp of both solve Functions: one launch of `method` (Batch.solution_jvp / solution_jvp_vel) on the input tangents."""
    batch = ctx.lease.batch
    (dots,) = _launch(batch, ctx.device, [(getattr(batch, method), tangents, 3, batch.n)], plain=True)
    return dots[0], dots[1], dots[2], None, None


class _MinTimeSolve(torch.autograd.Function):
    @staticmethod
    def forward(pos0, pos1, pos2, gap_tol, max_iter, params, holder):
        return _forward(holder, pos0, pos1, pos2, gap_tol, max_iter, params)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _setup_context(ctx, inputs, output)
        # the positions themselves, for the graph a create_graph backward builds (_SolutionVJP takes them as inputs); kept as
        # attributes, not saved tensors, so first-order use keeps its rules (no version check on the positions)
        ctx.pos = inputs[:3]

    @staticmethod
    def backward(ctx, g_vel1, g_dur0, g_dur1, _g_iters, _g_status):
        # one rp_batch_solution_vjp launch; differentiable once more (double backward) through _SolutionVJP
        bars = _SolutionVJP.apply(g_vel1, g_dur0, g_dur1, *ctx.pos, ctx.lease, ctx.device)
        return bars[0], bars[1], bars[2], None, None, None, None

    @staticmethod
    def jvp(ctx, t_pos0, t_pos1, t_pos2, _t_gap, _t_iter, _t_params, _t_holder):
        return _jvp(ctx, "solution_jvp", [t_pos0, t_pos1, t_pos2])


class _MinTimeSolveVel(torch.autograd.Function):
    """min_time_solve with end velocities: differentiable in (pos0, pos1, pos2, vel0, vel2), first order, through
    rp_batch_solution_vjp_vel (backward) and rp_batch_solution_jvp_vel (forward mode) at the state the solve left."""

    @staticmethod
    def forward(pos0, pos1, pos2, vel0, vel2, gap_tol, max_iter, params, holder):
        return _forward(holder, pos0, pos1, pos2, gap_tol, max_iter, params, vel=(vel0, vel2))

    @staticmethod
    def setup_context(ctx, inputs, output):
        _setup_context(ctx, inputs, output)
        ctx.has_vel = (inputs[3] is not None, inputs[4] is not None)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_vel1, g_dur0, g_dur1, _g_iters, _g_status):
        batch = ctx.lease.batch
        (bars,) = _launch(batch, ctx.device, [(batch.solution_vjp_vel, [g_vel1, g_dur0, g_dur1], 5, batch.n)])
        vel_bars = tuple(b if has else None for b, has in zip(bars[3:], ctx.has_vel))
        return (bars[0], bars[1], bars[2]) + vel_bars + (None, None, None, None)

    @staticmethod
    def jvp(ctx, t_pos0, t_pos1, t_pos2, t_vel0, t_vel2, _t_gap, _t_iter, _t_params, _t_holder):
        return _jvp(ctx, "solution_jvp_vel", [t_pos0, t_pos1, t_pos2, t_vel0, t_vel2])


class _SolutionVJP(torch.autograd.Function):
    """theta_bar = J^T g at the state of the leased batch (rp_batch_solution_vjp), as a function of the upstream gradients g and the
    positions theta, so that a backward run with create_graph=True can be differentiated again.  For cotangents h on theta_bar:
        g_bar = J h                      one rp_batch_solution_jvp launch
        pos_bar = S_a g_a H_a h          one rp_batch_solution_hessian launch and a contraction on the current stream
    ctx holds the lease: a graph built through this function keeps the batch out of the pool until the graph is freed."""

    @staticmethod
    def forward(ctx, g_vel1, g_dur0, g_dur1, pos0, pos1, pos2, lease, device):
        batch = lease.batch
        (bars,) = _launch(batch, device, [(batch.solution_vjp, [g_vel1, g_dur0, g_dur1], 3, batch.n)])
        ctx.lease = lease
        ctx.device = device
        ctx.save_for_backward(g_vel1, g_dur0, g_dur1)
        return bars[0], bars[1], bars[2]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, h_pos0, h_pos1, h_pos2):
        batch = ctx.lease.batch
        device = ctx.device
        gs = ctx.saved_tensors
        need_g, need_pos = any(ctx.needs_input_grad[:3]), any(ctx.needs_input_grad[3:6])
        hs = [h_pos0, h_pos1, h_pos2]
        n = batch.n
        g_bar = pos_bar = (None, None, None)
        if all(h is None for h in hs):
            return g_bar + pos_bar + (None, None)
        need_hess = need_pos and any(g is not None for g in gs)
        launches = []      # both in one ordered region
        if need_g:
            launches.append((batch.solution_jvp, hs, 3, n))
        if need_hess:
            launches.append((lambda d_hess: batch.solution_hessian(0, d_hess), [], 1, (n, 3, 3, 3)))
        results = _launch(batch, device, launches)
        if need_g:
            g_bar = tuple(results[0])
        if need_hess:
            (hess,) = results[-1]
            zero = torch.zeros(n, dtype=torch.float64, device=device)
            gv = torch.stack([g if g is not None else zero for g in gs], dim=1)
            hv = torch.stack([h if h is not None else zero for h in hs], dim=1)
            pb = torch.einsum("na,nabc,nc->bn", gv, hess, hv).contiguous()
            pos_bar = (pb[0], pb[1], pb[2])
        return g_bar + pos_bar + (None, None)


def min_time_solve(pos0, pos1, pos2, *, gap_tol=1e-8, max_iter=200, params=None, vel0=None, vel2=None):
    """Solve the F3 problems (pos0[i], pos1[i], pos2[i]) -- 1-D float64 tensors on one ROCm device -- on the current stream.

    Returns (vel1, duration0, duration1, iters, status): float64 tensors, differentiable with respect to the positions in reverse
    mode (backward, twice: create_graph=True gives a differentiable gradient) and forward mode (torch.autograd.forward_ad,
    torch.func.jvp), and the int32 step counts and RP_ST_* status words (not differentiable).  `params`: rp_params fields to override (a dict).  Derivatives are the implicit-function derivative at the
    state the solve returns (include/rp_batch.h, rp_batch_solution_vjp / rp_batch_solution_jvp): NaN for problems whose state is not
    finite or not strictly feasible.  Does not synchronise the host.

    vel0, vel2: end velocities (1-D float64 tensors on the positions' device; one given, the other counts as zeros) -- the problems are
    posed with rp_batch_set_problems_vel_device, and the outputs are differentiable in all five inputs, first order, in reverse and
    forward mode (rp_batch_solution_vjp_vel / _jvp_vel; NaN also where a duration is not positive); a double backward raises.  Large
    velocities can make the reference's model ill-posed: check `status`."""
    _check_positions(pos0, pos1, pos2)
    _check_params(params, "min_time_solve")
    if _check_velocities(pos0, vel0, vel2, "min_time_solve"):
        return _MinTimeSolveVel.apply(pos0, pos1, pos2, vel0, vel2, float(gap_tol), int(max_iter), params, _Holder())
    return _MinTimeSolve.apply(pos0, pos1, pos2, float(gap_tol), int(max_iter), params, _Holder())


def _solve_detached(who, pos0, pos1, pos2, gap_tol, max_iter, params, vel0, vel2, **which):
    """min_time_jacobian and min_time_hessian: the checks in `who`'s name, the solve on detached inputs with the launch `which`
    names (jacobian=True / hessian=True), the batch straight back to the pool."""
    _check_positions(pos0, pos1, pos2, who)
    _check_params(params, who)
    vel = (vel0, vel2) if _check_velocities(pos0, vel0, vel2, who) else None
    if vel is not None:
        vel = tuple(t.detach() if t is not None else None for t in vel)
    key, batch, outs = _solve(pos0.detach(), pos1.detach(), pos2.detach(), float(gap_tol), int(max_iter), params, vel=vel, **which)
    _pool.give(key, batch)      # the read-backs are enqueued; the next user of this key works on the same stream
    return outs


def min_time_jacobian(pos0, pos1, pos2, *, gap_tol=1e-8, max_iter=200, params=None, vel0=None, vel2=None):
    """min_time_solve's solve, and every problem's Jacobian at the state it returns, on the current stream.

    Returns (vel1, duration0, duration1, iters, status, jac) with jac (n, 3, 3) float64, jac[i, a, b] = d x_a / d pos_b of problem i
    for x = (vel1, duration0, duration1) (rp_batch_solution_jacobian; NaN rows as for min_time_solve's derivatives).  One solve and
    one Jacobian launch; nothing returned is differentiable.  Does not synchronise the host.  With end velocities (vel0= / vel2=, as
    min_time_solve's) jac is (n, 3, 5), columns (pos0, pos1, pos2, vel0, vel2) (rp_batch_solution_jacobian_vel)."""
    return _solve_detached("min_time_jacobian", pos0, pos1, pos2, gap_tol, max_iter, params, vel0, vel2, jacobian=True)


def min_time_hessian(pos0, pos1, pos2, *, gap_tol=1e-8, max_iter=200, params=None, vel0=None, vel2=None):
    """min_time_solve's solve, and every problem's Jacobian and second derivatives at the state it returns, on the current stream.

    Returns (vel1, duration0, duration1, iters, status, jac, hess) with jac (n, 3, 3) as min_time_jacobian's and hess (n, 3, 3, 3)
    float64, hess[i, a, b, c] = d^2 x_a / dpos_b dpos_c of problem i (rp_batch_solution_hessian; symmetric in b, c; NaN for the
    problems min_time_solve's derivatives are NaN for).  One solve and one Hessian launch; nothing returned is differentiable.  Does
    not synchronise the host.  With end velocities (vel0= / vel2=, as min_time_solve's) jac is min_time_jacobian's (n, 3, 5) and hess
    the second derivatives in the positions only, at that state (one Hessian and one Jacobian launch)."""
    return _solve_detached("min_time_hessian", pos0, pos1, pos2, gap_tol, max_iter, params, vel0, vel2, hessian=True)


# ---- the solved spline at the caller's own times ----
# (tables of eight tensors are in the C ABI's order: pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1)
def _check_trajectory(pos0, pos1, pos2, vel1, duration0, duration1, tau, vel0, vel2, who, queries="tau"):
    """The evaluator's arguments in the style of _check_positions; returns tau as (n, k) (a (k,) tau is broadcast).  `queries`: what the
    per-query argument is called in `who` (trajectory_crossing's is `level`; None: there is none to check here)."""
    _check_positions(pos0, pos1, pos2, who)
    for name, t in (("vel1", vel1), ("duration0", duration0), ("duration1", duration1)):
        _check_is_tensor(name, t, who)
        if t.device.type != "cuda" or t.device != pos0.device:
            raise TypeError(who + ": %s is on %s; it must be on the positions' ROCm device %s" % (name, t.device, pos0.device))
        _check_is_float64(name, t, who)
        if t.shape != pos0.shape:
            raise ValueError(who + ": %s has shape %s, the positions %s" % (name, tuple(t.shape), tuple(pos0.shape)))
    _check_velocities(pos0, vel0, vel2, who)
    return _check_tau(pos0, tau, who, queries) if queries is not None else None


def _check_tau(pos0, tau, who, name="tau"):
    """tau (or, under another name, the levels of trajectory_crossing) against the (checked) positions; returns it as (n, k) (a (k,) tau
    is broadcast)."""
    _check_is_tensor(name, tau, who)
    if tau.device.type != "cuda" or tau.device != pos0.device:
        raise TypeError(who + ": %s is on %s; it must be on the positions' ROCm device %s" % (name, tau.device, pos0.device))
    _check_is_float64(name, tau, who)
    n = pos0.shape[0]
    if tau.dim() == 1 and tau.shape[0] > 0:
        return tau.unsqueeze(0).expand(n, tau.shape[0])
    if tau.dim() != 2 or tau.shape[0] != n or tau.shape[1] == 0:
        raise ValueError(who + ": %s must have shape (%d, k) or (k,) with k >= 1, got %s" % (name, n, tuple(tau.shape)))
    return tau


# What the query Functions below share: _enqueue is the one launch, _keep and _kept what a ctx holds, _query_shape
# the shape of the outputs, _empty and _bars the buffers a launch writes, _class_masks the class of a time.
def _enqueue(entry, device, *args):
    """One launch of a capi entry on the current stream of `device`, no host synchronisation.  args: what the entry takes behind the
    device and the stream, in its order (the sizes n, k[, m, d] included) -- an int goes as it is, a tensor as its address (the one
    under torch.func's wrappers: _plain), None as NULL, a list or tuple of tensors and Nones as a table of addresses."""
    addr = lambda t: _plain(t).data_ptr() if t is not None else 0      # noqa: E731
    with torch.cuda.device(device):      # the entry selects the device for its thread: put torch's choice back afterwards
        entry(device.index, torch.cuda.current_stream(device).cuda_stream,
              *[a if isinstance(a, int) else [addr(t) for t in a] if isinstance(a, (list, tuple)) else addr(a) for a in args])


def _dense(t):
    return t.contiguous() if t is not None else None


def _empty(shape, device):
    return torch.empty(shape, dtype=torch.float64, device=device)


def _bars(need, shape, device):
    """A buffer of `shape` for every flag of `need` that holds, None for the others: what a derivative launch is asked to form."""
    return [_empty(shape, device) if wanted else None for wanted in need]


def _query_shape(n, *queries):
    """(n, k) of a query's outputs: the shape of the first per-query argument that was given, (n, 1) if none was."""
    for t in queries:
        if t is not None:
            return t.shape
    return (n, 1)


def _keep(ctx, inputs, outputs=(), dead=(), given=None, forward=True):
    """setup_context of the query Functions: keeps those of `inputs` that `given` flags (None: those that are not None) and `outputs`, for
    backward and, unless forward=False, for jvp; `dead` are the outputs that are not differentiable.  Gradients are not materialised: an
    output the loss does not use arrives in backward as None and goes to the kernel as NULL, which it does not read."""
    ctx.set_materialize_grads(False)
    if dead:
        ctx.mark_non_differentiable(*dead)
    ctx.given = given if given is not None else [t is not None for t in inputs]
    kept = [t for t, has in zip(inputs, ctx.given) if has] + list(outputs)
    ctx.save_for_backward(*kept)
    if forward:
        ctx.save_for_forward(*kept)


def _kept(ctx):
    """What _keep kept: (the inputs, None back in the places of those not kept; the outputs)"""
    kept = iter(ctx.saved_tensors)
    return [next(kept) if has else None for has in ctx.given], list(kept)


def _class_masks(t, missing, tests, last_only=None):
    """The class of each time: where t equals tests[0], else tests[1], ... (None: nowhere) -- exclusive, in that priority, never where
    missing; the last class only where last_only holds."""
    masks, taken = [], missing
    for at, ref in enumerate(tests):
        mask = (t == ref) & ~taken if ref is not None else torch.zeros_like(missing)
        if last_only is not None and at == len(tests) - 1:
            mask = mask & last_only
        masks.append(mask)
        taken = taken | mask
    return masks


def _axis_tables(inputs, d, vehicles=2):
    """inputs[:8 d vehicles] -- vehicle-major, then axis-major, each axis in the table's order -- as one list per vehicle of its d lists of
    eight dense tensors."""
    return [[[_dense(t) for t in inputs[8 * (v * d + c):8 * (v * d + c) + 8]] for c in range(d)] for v in range(vehicles)]


def _pair_gaps(a, b, t_a, t_b):
    """The d gaps D_c = pos_Ac(t_a) - pos_Bc(t_b) of two vehicles of d axes: one evaluator launch on each axis' two splines"""
    gaps = []
    for sa, sb in zip(a, b):
        pa, pb = _empty(t_a.shape, t_a.device), _empty(t_a.shape, t_a.device)
        _enqueue(capi.trajectory_eval, t_a.device, *t_a.shape, sa, t_a, pa, None, None)
        _enqueue(capi.trajectory_eval, t_a.device, *t_a.shape, sb, t_b, pb, None, None)
        gaps.append(pa - pb)
    return gaps


def _eval_vjp(spline, tau, g, need):
    """The one rp_trajectory_eval_vjp launch of _TrajectoryEval.backward and _TrajectoryVJP.forward: the eight bars and tau_bar that
    `need` names, None for the others."""
    bars = _bars(need[:8], tau.shape[0], tau.device)
    tau_bar = _empty(tau.shape, tau.device) if need[8] else None
    _enqueue(capi.trajectory_eval_vjp, tau.device, *tau.shape, spline, tau, *[_dense(x) for x in g], bars, tau_bar)
    return tuple(bars) + (tau_bar,)


def _backward2(ctx, vjp, g, *more):
    """backward of the three order=2 Functions: the first-order launch made through `vjp`, so that a create_graph backward records it."""
    count = len(ctx.given)
    if all(x is None for x in g):
        return (None,) * count
    return vjp.apply(*_kept(ctx)[0], *g, tuple(ctx.needs_input_grad[:count]), *more)


class _TrajectoryEval(torch.autograd.Function):
    """(pos, vel, acc) of the spline at tau: differentiable to first order in the eight spline inputs (the table's order) and in tau."""

    @staticmethod
    def forward(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, tau):
        spline = [_dense(t) for t in (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1)]
        tau = tau.contiguous()
        outs = [_empty(tau.shape, tau.device) for _ in range(3)]
        _enqueue(capi.trajectory_eval, tau.device, *tau.shape, spline, tau, *outs)
        return tuple(outs)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _keep(ctx, inputs)

    @staticmethod
    def _inputs(ctx):
        inputs, _ = _kept(ctx)
        return [_dense(t) for t in inputs[:8]], inputs[8].contiguous()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g):
        if all(x is None for x in g):
            return (None,) * 9
        spline, tau = _TrajectoryEval._inputs(ctx)
        return _eval_vjp(spline, tau, g, ctx.needs_input_grad)

    @staticmethod
    def jvp(ctx, *tangents):
        spline, tau = _TrajectoryEval._inputs(ctx)
        dots = [_dense(t) for t in tangents]
        outs = [_empty(tau.shape, tau.device) for _ in range(3)]
        _enqueue(capi.trajectory_eval_jvp, tau.device, *tau.shape, spline, tau, dots[:8], dots[8], *outs)
        return tuple(outs)


class _TrajectoryEval2(_TrajectoryEval):
    """_TrajectoryEval with a backward that can be differentiated again (order=2): the same forward, the same forward-mode rule, and
    the same one rp_trajectory_eval_vjp launch in backward, made through _TrajectoryVJP so that a create_graph backward records it."""

    @staticmethod
    def backward(ctx, *g):
        return _backward2(ctx, _TrajectoryVJP, g)


class _TrajectoryVJP(torch.autograd.Function):
    """(the eight spline inputs, tau, g_pos, g_vel, g_acc) -> (the eight bars, tau_bar): one rp_trajectory_eval_vjp launch that forms the
    bars `need` names (the others are None), as a function that can be differentiated once.  For cotangents u on its outputs:
        (g_pos, g_vel, g_acc)_bar = J u                          one rp_trajectory_eval_jvp launch with tangents u
        (spline, tau)_bar = (S_o g_o (second derivative of o)) u   one rp_trajectory_eval_hvp launch with direction u (symmetric)
    each made only if something on its side requires grad."""

    @staticmethod
    def forward(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, tau, g_pos, g_vel, g_acc, need):
        spline = [_dense(t) for t in (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1)]
        return _eval_vjp(spline, tau.contiguous(), (g_pos, g_vel, g_acc), need)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _keep(ctx, inputs[:12], forward=False)      # (a bar nothing downstream uses arrives as None too)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *u):
        out = [None] * 13
        if all(x is None for x in u):
            return tuple(out)
        inputs, _ = _kept(ctx)
        spline, tau, g = [_dense(t) for t in inputs[:8]], inputs[8].contiguous(), [_dense(t) for t in inputs[9:12]]
        need, dev = ctx.needs_input_grad, tau.device
        dots, tau_dot = [_dense(x) for x in u[:8]], _dense(u[8])
        if any(need[9:12]):
            outs = _bars(need[9:12], tau.shape, dev)
            _enqueue(capi.trajectory_eval_jvp, dev, *tau.shape, spline, tau, dots, tau_dot, *outs)
            out[9:12] = outs
        if any(need[:9]) and any(x is not None for x in g):
            bars = _bars(need[:8], tau.shape[0], dev)
            tau_bar = _empty(tau.shape, dev) if need[8] else None
            _enqueue(capi.trajectory_eval_hvp, dev, *tau.shape, spline, tau, *g, dots, tau_dot, bars, tau_bar)
            out[:9] = bars + [tau_bar]
        return tuple(out)


def _check_order(order, who):
    if order not in (1, 2):
        raise ValueError("%s: order must be 1 or 2, got %r" % (who, order))


def trajectory_eval(pos0, pos1, pos2, vel1, duration0, duration1, tau, *, vel0=None, vel2=None, order=1):
    """Position, velocity and acceleration of the two-segment spline (pos0, vel0) -> (pos1, vel1) -> (pos2, vel2) with the durations
    duration0, duration1 -- 1-D float64 tensors on one ROCm device; vel0 / vel2 of None count as zeros -- at the times tau, (n, k) or
    (k,) (the same times for every problem), counted from the start of segment 0.  Returns (pos, vel, acc), (n, k) each.

    One rp_trajectory_eval launch on the current stream (include/rp_batch.h: tau < duration0 selects segment 0; no clamping, outside
    [0, duration0 + duration1] the end segments' cubics continue; a problem with a duration that is not finite or not > 0 is NaN).
    Differentiable to first order in all eight spline inputs and in tau: reverse mode is one rp_trajectory_eval_vjp launch (tau's
    gradient is formed only when tau requires it; a double backward raises torch's once_differentiable error), forward mode
    (torch.autograd.forward_ad, torch.func.jvp) one rp_trajectory_eval_jvp launch.  Does not synchronise the host.

    order=2 (1 or 2; anything else: ValueError) makes the backward differentiable once more -- torch.autograd.grad(..., create_graph=True),
    torch.autograd.functional.hvp / hessian: the values, the gradients and the forward-mode tangents are the same launches and the same
    bits as with order=1; the backward of the backward is one rp_trajectory_eval_jvp launch (for the gradients in the first backward's
    grad_outputs) and one rp_trajectory_eval_hvp launch (for those in the spline inputs and tau), each only if something on its side
    requires grad.  A third derivative raises torch's once_differentiable error."""
    _check_order(order, "trajectory_eval")
    tau = _check_trajectory(pos0, pos1, pos2, vel1, duration0, duration1, tau, vel0, vel2, "trajectory_eval")
    function = _TrajectoryEval if order == 1 else _TrajectoryEval2
    return function.apply(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, tau)


def min_time_trajectory(pos0, pos1, pos2, tau, *, normalized=False, vel0=None, vel2=None, gap_tol=1e-8, max_iter=200, params=None, order=1):
    """min_time_solve, then trajectory_eval of its solution at tau ((n, k) or (k,)): returns (pos, vel, acc, vel1, duration0, duration1,
    iters, status).  normalized=True: tau is a fraction of each problem's total time (0: the start, 1: the end), multiplied by
    duration0 + duration1 in torch, so that its dependence on the solution is differentiated too.  Plain composition: pos, vel and acc
    are differentiable in the positions, the end velocities and tau through the solve's derivatives and the evaluator's.

    order=2 (trajectory_eval's): with the solve's own double backward, pos, vel and acc are twice differentiable in the positions and tau
    for rest-to-rest problems (normalized=True included: a torch multiplication).  With vel0 / vel2 that require grad the solve is first
    order, and a double backward through it raises torch's once_differentiable error as it does with order=1."""
    _check_order(order, "min_time_trajectory")
    _check_positions(pos0, pos1, pos2, "min_time_trajectory")
    tau = _check_tau(pos0, tau, "min_time_trajectory")      # before the solve: a bad tau costs none
    vel1, duration0, duration1, iters, status = min_time_solve(pos0, pos1, pos2, gap_tol=gap_tol, max_iter=max_iter, params=params,
                                                                vel0=vel0, vel2=vel2)
    if normalized:
        tau = tau * (duration0 + duration1).unsqueeze(1)
    pos, vel, acc = trajectory_eval(pos0, pos1, pos2, vel1, duration0, duration1, tau, vel0=vel0, vel2=vel2, order=order)
    return pos, vel, acc, vel1, duration0, duration1, iters, status


# ---- the inverse: when the spline first reaches a level ----
class _TrajectoryCrossing(torch.autograd.Function):
    """(time, vel) of the first crossing of each level: time differentiable to first order in the eight spline inputs (the table's order)
    and in the level, through the evaluator's derivative launches -- pos(theta, time) = level gives
    d time = (d level - d pos at fixed time) / vel.  vel is for the backward and is not differentiable."""

    @staticmethod
    def forward(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, level):
        spline = [_dense(t) for t in (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1)]
        level = level.contiguous()
        time, vel = _empty(level.shape, level.device), _empty(level.shape, level.device)
        _enqueue(capi.trajectory_crossing, level.device, *level.shape, spline, level, time, vel)
        return time, vel

    @staticmethod
    def setup_context(ctx, inputs, output):
        _keep(ctx, inputs[:8], output, dead=output[1:])      # the level itself is in neither derivative

    @staticmethod
    def _saved(ctx):
        """(the eight spline tensors, the times with 0 where no crossing exists, vel, where no crossing exists)"""
        spline, (time, vel) = _kept(ctx)
        missing = torch.isnan(time)
        return [_dense(t) for t in spline], torch.where(missing, torch.zeros_like(time), time), vel, missing

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_time, _g_vel):
        if g_time is None:
            return (None,) * 9
        spline, tau, vel, missing = _TrajectoryCrossing._saved(ctx)
        w = torch.where(missing, torch.zeros_like(tau), g_time / vel)      # an unreached level: gradient 0
        bars = _bars(ctx.needs_input_grad[:8], tau.shape[0], tau.device)
        if any(b is not None for b in bars):
            _enqueue(capi.trajectory_eval_vjp, tau.device, *tau.shape, spline, tau, -w, None, None, bars, None)
        return tuple(bars) + (w if ctx.needs_input_grad[8] else None,)

    @staticmethod
    def jvp(ctx, *tangents):
        spline, tau, vel, missing = _TrajectoryCrossing._saved(ctx)
        dots = [_dense(t) for t in tangents[:8]]
        pos_dot = _empty(tau.shape, tau.device)
        _enqueue(capi.trajectory_eval_jvp, tau.device, *tau.shape, spline, tau, dots, None, pos_dot, None, None)
        level_dot = tangents[8] if tangents[8] is not None else torch.zeros_like(tau)
        time_dot = torch.where(missing, torch.full_like(tau, float("nan")), (level_dot - pos_dot) / vel)
        return time_dot, None


def trajectory_crossing(pos0, pos1, pos2, vel1, duration0, duration1, level, *, vel0=None, vel2=None):
    """The first time in [0, duration0 + duration1] at which the spline of trajectory_eval is at each level -- level (n, k), or (k,) for
    the same levels in every problem -- counted from the start of segment 0: (n, k), NaN where the spline does not reach the level (no
    extrapolation).  The inverse of trajectory_eval's pos.

    One rp_trajectory_crossing launch on the current stream (include/rp_batch.h: the first of the spline's six monotone pieces that holds
    the level, then a bracketed Newton search with a fixed trip bound; a problem with a duration that is not finite or not > 0 is NaN, a
    NaN level is NaN for itself; a level within rounding of an extremum of pos may give the touch, a later crossing, or NaN).
    Differentiable to first order in all eight spline inputs and in the level, d time = (d level - d pos) / vel: reverse mode is one
    rp_trajectory_eval_vjp launch, forward mode one rp_trajectory_eval_jvp launch; a double backward raises
    torch's once_differentiable error.  An unreached level has gradient 0 (forward mode: NaN, as the time); where the velocity at the
    crossing is 0 (a touch) there is no derivative and the result is inf or NaN.  Does not synchronise the host."""
    level = _check_trajectory(pos0, pos1, pos2, vel1, duration0, duration1, level, vel0, vel2, "trajectory_crossing", "level")
    return _TrajectoryCrossing.apply(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, level)[0]


def min_time_crossing(pos0, pos1, pos2, level, *, vel0=None, vel2=None, gap_tol=1e-8, max_iter=200, params=None):
    """min_time_solve, then trajectory_crossing of its solution at level ((n, k) or (k,)): returns (time, vel1, duration0, duration1, iters,
    status).  Plain composition: time is differentiable in the positions, the end velocities and the level through the solve's
    derivatives and the crossing's."""
    _check_positions(pos0, pos1, pos2, "min_time_crossing")
    level = _check_tau(pos0, level, "min_time_crossing", "level")      # before the solve: a bad level costs none
    vel1, duration0, duration1, iters, status = min_time_solve(pos0, pos1, pos2, gap_tol=gap_tol, max_iter=max_iter, params=params,
                                                                vel0=vel0, vel2=vel2)
    time = trajectory_crossing(pos0, pos1, pos2, vel1, duration0, duration1, level, vel0=vel0, vel2=vel2)
    return time, vel1, duration0, duration1, iters, status


# ---- how far and how fast at most: the extreme position and velocity over a window ----
class _TrajectoryExtrema(torch.autograd.Function):
    """(pos_min, pos_max, vel_min, vel_max, and a time at which each is attained) over the windows [lo, hi] clamped to the spline: the values
    differentiable to first order in the eight spline inputs (the table's order) and in lo and hi, through the evaluator's derivative
    launches at the returned times.  Each time is classified by equality -- lo, else hi, else duration0 + duration1, else duration0, else
    interior -- and the evaluator's derivative in the time goes to that input: to nothing at an interior time, where the value is
    stationary (the envelope theorem).  The times are not differentiable."""

    @staticmethod
    def forward(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, lo, hi):
        spline = [_dense(t) for t in (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1)]
        lo, hi = _dense(lo), _dense(hi)
        n, k = _query_shape(pos0.shape[0], lo, hi)
        outs = [_empty((n, k), pos0.device) for _ in range(8)]
        _enqueue(capi.trajectory_extrema, pos0.device, n, k, spline, lo, hi, outs[:4], outs[4:])
        return tuple(outs)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _keep(ctx, inputs, output, dead=output[4:])

    @staticmethod
    def _saved(ctx):
        """(the eight spline tensors; the four times side by side, (n, 4 k), 0 where the value is NaN; where it is NaN; the class masks
        LO, HI, END, KNOT of each time, exclusive and in that priority)"""
        inputs, outs = _kept(ctx)
        spline, lo, hi = [_dense(t) for t in inputs[:8]], inputs[8], inputs[9]
        time = torch.cat(outs[4:], dim=1)
        missing = torch.isnan(torch.cat(outs[:4], dim=1)) | torch.isnan(time)
        t0 = torch.where(missing, torch.zeros_like(time), time)
        d0, T = spline[6].unsqueeze(1), (spline[6] + spline[7]).unsqueeze(1)
        wide = lambda t: t.repeat(1, 4) if t is not None else None      # noqa: E731
        return spline, t0, missing, _class_masks(t0, missing, [wide(lo), wide(hi), T, d0])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g0, g1, g2, g3, *_g_times):
        if g0 is None and g1 is None and g2 is None and g3 is None:
            return (None,) * 10
        spline, t0, missing, (is_lo, is_hi, is_end, is_knot) = _TrajectoryExtrema._saved(ctx)
        n, k = t0.shape[0], t0.shape[1] // 4
        zero = torch.zeros((n, k), dtype=torch.float64, device=t0.device)
        part = lambda g: g if g is not None else zero      # noqa: E731
        g_pos = torch.cat([part(g0), part(g1), zero, zero], dim=1)
        g_vel = torch.cat([zero, zero, part(g2), part(g3)], dim=1)
        g_pos = torch.where(missing, torch.zeros_like(g_pos), g_pos)      # a NaN value: gradient 0
        g_vel = torch.where(missing, torch.zeros_like(g_vel), g_vel)
        need = ctx.needs_input_grad
        bars = _bars(need[:8], n, t0.device)
        want_tau = need[6] or need[7] or need[8] or need[9]
        tau_bar = _empty(t0.shape, t0.device) if want_tau else None
        _enqueue(capi.trajectory_eval_vjp, t0.device, *t0.shape, spline, t0, g_pos, g_vel, None, bars, tau_bar)
        lo_bar = hi_bar = None
        if want_tau:
            routed = lambda mask: torch.where(mask, tau_bar, torch.zeros_like(tau_bar))      # noqa: E731
            fold = lambda x: x.reshape(n, 4, k).sum(dim=1)      # noqa: E731
            end = routed(is_end).sum(dim=1)
            if need[6]:
                bars[6] = bars[6] + (end + routed(is_knot).sum(dim=1))
            if need[7]:
                bars[7] = bars[7] + end
            if need[8]:
                lo_bar = fold(routed(is_lo))
            if need[9]:
                hi_bar = fold(routed(is_hi))
        return tuple(bars) + (lo_bar, hi_bar)

    @staticmethod
    def jvp(ctx, *tangents):
        spline, t0, missing, (is_lo, is_hi, is_end, is_knot) = _TrajectoryExtrema._saved(ctx)
        n, k = t0.shape[0], t0.shape[1] // 4
        dots = [_dense(t) for t in tangents[:8]]
        tau_dot = torch.zeros_like(t0)
        col = lambda t: t.unsqueeze(1).expand(n, 4 * k) if t is not None else None      # noqa: E731
        d0_dot, d1_dot = col(dots[6]), col(dots[7])
        if tangents[8] is not None:
            tau_dot = torch.where(is_lo, tangents[8].repeat(1, 4), tau_dot)
        if tangents[9] is not None:
            tau_dot = torch.where(is_hi, tangents[9].repeat(1, 4), tau_dot)
        if d0_dot is not None:
            tau_dot = torch.where(is_end | is_knot, d0_dot, tau_dot)
        if d1_dot is not None:
            tau_dot = torch.where(is_end, tau_dot + d1_dot, tau_dot)
        pos_dot, vel_dot = _empty(t0.shape, t0.device), _empty(t0.shape, t0.device)
        _enqueue(capi.trajectory_eval_jvp, t0.device, *t0.shape, spline, t0, dots, tau_dot.contiguous(), pos_dot, vel_dot, None)
        nan = torch.full_like(t0, float("nan"))
        pos_dot, vel_dot = torch.where(missing, nan, pos_dot), torch.where(missing, nan, vel_dot)
        return tuple(x.clone() for x in (pos_dot[:, :k], pos_dot[:, k:2 * k], vel_dot[:, 2 * k:3 * k], vel_dot[:, 3 * k:])) + (None,) * 4


def _check_window(pos0, lo, hi, who):
    """lo and hi (None: -inf / +inf) against the (checked) positions, each like tau; both given: the same shape after broadcasting."""
    lo = _check_tau(pos0, lo, who, "lo") if lo is not None else None
    hi = _check_tau(pos0, hi, who, "hi") if hi is not None else None
    if lo is not None and hi is not None and lo.shape != hi.shape:
        raise ValueError(who + ": lo has shape %s, hi %s" % (tuple(lo.shape), tuple(hi.shape)))
    return lo, hi


def trajectory_extrema(pos0, pos1, pos2, vel1, duration0, duration1, lo=None, hi=None, *, vel0=None, vel2=None):
    """The extreme position and velocity of the spline of trajectory_eval over the windows of time [lo, hi] -- (n, k), or (k,) for the same
    windows in every problem; None: -inf / +inf, both None: k = 1, the whole spline -- clamped to [0, duration0 + duration1] (no
    extrapolation).  Returns (pos_min, pos_max, vel_min, vel_max, t_pos_min, t_pos_max, t_vel_min, t_vel_max), (n, k) each: the values and a
    time at which each is attained.  NaN where the clamped window is empty (a NaN end, a window wholly outside the spline).

    One rp_trajectory_extrema launch on the current stream (include/rp_batch.h: the candidates are the window's ends, the knot and the
    stationary points strictly inside; the earliest among equal values wins; a value is bit for bit trajectory_eval's at the returned
    time).  The values are differentiable to first order in all eight spline inputs and in lo and hi: reverse mode is one
    rp_trajectory_eval_vjp launch, forward mode one rp_trajectory_eval_jvp launch, at the returned times; a double
    backward raises torch's once_differentiable error.  At a tie between candidates, and where a window end is clamped, the derivative is
    that of the branch the forward pass found.  A NaN value has gradient 0 (forward mode: NaN).  The times are not differentiable.  Does
    not synchronise the host."""
    who = "trajectory_extrema"
    _check_trajectory(pos0, pos1, pos2, vel1, duration0, duration1, None, vel0, vel2, who, None)
    lo, hi = _check_window(pos0, lo, hi, who)
    return _TrajectoryExtrema.apply(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, lo, hi)


def min_time_extrema(pos0, pos1, pos2, lo=None, hi=None, *, vel0=None, vel2=None, gap_tol=1e-8, max_iter=200, params=None):
    """min_time_solve, then trajectory_extrema of its solution over [lo, hi] ((n, k), (k,) or None): returns the eight of
    trajectory_extrema, then (vel1, duration0, duration1, iters, status).  Plain composition: the values are differentiable in the
    positions, the end velocities and the window's ends through the solve's derivatives and the extrema's."""
    _check_positions(pos0, pos1, pos2, "min_time_extrema")
    lo, hi = _check_window(pos0, lo, hi, "min_time_extrema")      # before the solve: a bad window costs none
    vel1, duration0, duration1, iters, status = min_time_solve(pos0, pos1, pos2, gap_tol=gap_tol, max_iter=max_iter, params=params,
                                                                vel0=vel0, vel2=vel2)
    out = trajectory_extrema(pos0, pos1, pos2, vel1, duration0, duration1, lo, hi, vel0=vel0, vel2=vel2)
    return tuple(out) + (vel1, duration0, duration1, iters, status)


# ---- how close two splines get: the extreme gap over a window ----
class _TrajectoryGap(torch.autograd.Function):
    """(gap_min, gap_max, and a time at which each is attained) of pos_A(t) - pos_B(t - delay) over the windows [lo, hi] clamped to the two
    splines' common domain: the values differentiable to first order in the sixteen spline inputs (A's table, then B's), in lo, hi and the
    delay, through the evaluator's derivative launches on each spline at the returned times.  Each time is classified by equality -- lo,
    hi, A's end, B's end, A's knot, B's knot, the delayed start, else a clamped +0.0 or a stationary point -- and the derivative in the
    time goes to the inputs that time is made of.  The times are not differentiable."""

    @staticmethod
    def forward(*inputs):
        a, b = [_dense(t) for t in inputs[:8]], [_dense(t) for t in inputs[8:16]]
        lo, hi, delay = (_dense(t) for t in inputs[16:19])
        n, k = _query_shape(inputs[0].shape[0], lo, hi, delay)
        device = inputs[0].device
        outs = [_empty((n, k), device) for _ in range(4)]
        _enqueue(capi.trajectory_gap, device, n, k, a, b, lo, hi, delay, outs[:2], outs[2:])
        return tuple(outs)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _keep(ctx, inputs, output, dead=output[2:])

    @staticmethod
    def _saved(ctx):
        """(A's and B's eight tensors; the two times side by side, (n, 2 k), 0 where the value is NaN, and B's, those minus the delay;
        where it is NaN; the class masks LO, HI, END_A, END_B, KNOT_A, KNOT_B, START of each time, exclusive and in that priority)"""
        inputs, outs = _kept(ctx)
        a, b = [_dense(t) for t in inputs[:8]], [_dense(t) for t in inputs[8:16]]
        lo, hi, delay = inputs[16:19]
        time = torch.cat(outs[2:], dim=1)
        missing = torch.isnan(torch.cat(outs[:2], dim=1)) | torch.isnan(time)
        zero = torch.zeros_like(time)
        t_a = torch.where(missing, zero, time)
        shift = delay.repeat(1, 2) if delay is not None else zero
        t_b = torch.where(missing, zero, t_a - shift)
        tests = ((lo.repeat(1, 2) if lo is not None else None), (hi.repeat(1, 2) if hi is not None else None),
                 (a[6] + a[7]).unsqueeze(1), shift + (b[6] + b[7]).unsqueeze(1), a[6].unsqueeze(1), shift + b[6].unsqueeze(1), shift)
        masks = _class_masks(t_a, missing, tests, last_only=shift > 0)      # a start clamped to +0.0 is a constant
        return a, b, t_a.contiguous(), t_b.contiguous(), missing, masks

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_min, g_max, *_g_times):
        if g_min is None and g_max is None:
            return (None,) * 19
        a, b, t_a, t_b, missing, (is_lo, is_hi, end_a, end_b, knot_a, knot_b, start) = _TrajectoryGap._saved(ctx)
        n, k = t_a.shape[0], t_a.shape[1] // 2
        zero = torch.zeros((n, k), dtype=torch.float64, device=t_a.device)
        g = torch.cat([g_min if g_min is not None else zero, g_max if g_max is not None else zero], dim=1)
        g = torch.where(missing, torch.zeros_like(g), g)      # a NaN value: gradient 0
        need = ctx.needs_input_grad
        want_time = need[6] or need[7] or need[14] or need[15] or need[16] or need[17] or need[18]
        bars, tau_bars = [], []
        for first, spline, tau, g_pos in ((0, a, t_a, g), (8, b, t_b, -g)):
            bar = _bars(need[first:first + 8], n, tau.device)
            tau_bar = _empty(tau.shape, tau.device) if want_time else None
            if want_time or any(x is not None for x in bar):
                _enqueue(capi.trajectory_eval_vjp, tau.device, *tau.shape, spline, tau, g_pos.contiguous(), None, None, bar, tau_bar)
            bars += bar
            tau_bars.append(tau_bar)
        lo_bar = hi_bar = delay_bar = None
        if want_time:
            time_bar = tau_bars[0] + tau_bars[1]
            routed = lambda mask: torch.where(mask, time_bar, torch.zeros_like(time_bar))      # noqa: E731
            fold = lambda x: x.reshape(n, 2, k).sum(dim=1)      # noqa: E731
            for f, masks in ((6, (end_a, knot_a)), (7, (end_a,)), (14, (end_b, knot_b)), (15, (end_b,))):
                if need[f]:
                    bars[f] = bars[f] + sum(routed(m).sum(dim=1) for m in masks)
            if need[16]:
                lo_bar = fold(routed(is_lo))
            if need[17]:
                hi_bar = fold(routed(is_hi))
            if need[18]:      # B is at time - delay, and the times that hold the delay move with it
                delay_bar = fold(routed(end_b | knot_b | start) - tau_bars[1])
        return tuple(bars) + (lo_bar, hi_bar, delay_bar)

    @staticmethod
    def jvp(ctx, *tangents):
        a, b, t_a, t_b, missing, (is_lo, is_hi, end_a, end_b, knot_a, knot_b, start) = _TrajectoryGap._saved(ctx)
        n, k = t_a.shape[0], t_a.shape[1] // 2
        dots = [_dense(t) for t in tangents[:16]]
        zero = torch.zeros_like(t_a)
        col = lambda t: t.unsqueeze(1).expand(n, 2 * k) if t is not None else zero      # noqa: E731
        wide = lambda t: t.repeat(1, 2) if t is not None else zero      # noqa: E731
        delay_dot = wide(tangents[18])
        time_dot = torch.where(is_lo, wide(tangents[16]), zero)
        time_dot = torch.where(is_hi, wide(tangents[17]), time_dot)
        time_dot = torch.where(end_a, col(dots[6]) + col(dots[7]), time_dot)
        time_dot = torch.where(end_b, delay_dot + col(dots[14]) + col(dots[15]), time_dot)
        time_dot = torch.where(knot_a, col(dots[6]), time_dot)
        time_dot = torch.where(knot_b, delay_dot + col(dots[14]), time_dot)
        time_dot = torch.where(start, delay_dot, time_dot)
        pos_a, pos_b = _empty(t_a.shape, t_a.device), _empty(t_a.shape, t_a.device)
        _enqueue(capi.trajectory_eval_jvp, t_a.device, *t_a.shape, a, t_a, dots[:8], time_dot.contiguous(), pos_a, None, None)
        _enqueue(capi.trajectory_eval_jvp, t_a.device, *t_a.shape, b, t_b, dots[8:], (time_dot - delay_dot).contiguous(), pos_b, None, None)
        gap_dot = torch.where(missing, torch.full_like(t_a, float("nan")), pos_a - pos_b)
        return gap_dot[:, :k].clone(), gap_dot[:, k:].clone(), None, None


def _check_spline_arg(name, spline, who):
    """One vehicle's spline as trajectory_gap takes it: a sequence of six tensors (pos0, pos1, pos2, vel1, duration0, duration1) or of
    eight, with (vel0, vel2) appended (either may be None: zeros)."""
    if not isinstance(spline, (list, tuple)):
        raise TypeError("%s: %s must be a list or tuple of six or eight tensors, got %s" % (who, name, type(spline).__name__))
    if len(spline) not in (6, 8):
        raise ValueError("%s: %s must hold six tensors (pos0, pos1, pos2, vel1, duration0, duration1) or eight (vel0, vel2 appended), got %d"
                         % (who, name, len(spline)))


def _spline_table(name, spline, who):
    """The (checked) sequence's tensors checked as trajectory_eval's arguments; returns the eight in the C ABI's table order."""
    pos0, pos1, pos2, vel1, duration0, duration1 = spline[:6]
    vel0, vel2 = spline[6:] if len(spline) == 8 else (None, None)
    _check_trajectory(pos0, pos1, pos2, vel1, duration0, duration1, None, vel0, vel2, "%s: %s" % (who, name), None)
    return [pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1]


def _check_named_queries(pos0, named, who):
    """Optional per-query arguments, (name, tensor or None) each, against the (checked) positions, each like tau; those given: one shape
    after broadcasting."""
    given = [(name, _check_tau(pos0, t, who, name) if t is not None else None) for name, t in named]
    shapes = [(name, t.shape) for name, t in given if t is not None]
    for name, shape in shapes[1:]:
        if shape != shapes[0][1]:
            raise ValueError(who + ": %s has shape %s, %s %s" % (shapes[0][0], tuple(shapes[0][1]), name, tuple(shape)))
    return [t for _, t in given]


def _check_gap_queries(pos0, lo, hi, delay, who):
    """lo, hi (None: -inf / +inf) and delay (None: 0)."""
    return _check_named_queries(pos0, (("lo", lo), ("hi", hi), ("delay", delay)), who)


def _check_same_batch(pos_a, pos_b, who):
    if pos_b.device != pos_a.device:
        raise TypeError(who + ": b is on %s; it must be on a's ROCm device %s" % (pos_b.device, pos_a.device))
    if pos_b.shape != pos_a.shape:
        raise ValueError(who + ": a holds %d problems, b %d" % (pos_a.shape[0], pos_b.shape[0]))


def trajectory_gap(a, b, lo=None, hi=None, delay=None):
    """The extreme gap between two splines of trajectory_eval in one frame, D(t) = pos_a(t) - pos_b(t - delay), over the windows of time
    [lo, hi].  a, b: each a sequence of six tensors (pos0, pos1, pos2, vel1, duration0, duration1), or of eight with (vel0, vel2) appended,
    of the same n on the same ROCm device.  lo, hi, delay: (n, k), or (k,) for the same queries in every problem; None: -inf / +inf / 0,
    all three None: k = 1, the whole common domain.  b's clock starts `delay` after a's; no extrapolation: the window is clamped to
    [max(delay, 0), min(T_a, delay + T_b)].  Returns (gap_min, gap_max, t_gap_min, t_gap_max), (n, k) each: the values and a time (on a's
    clock) at which each is attained; NaN where the clamped window is empty, where the delay is NaN or infinite, and for a problem either
    of whose splines has a duration that is not finite or not > 0.  The unsigned separation: torch.clamp(torch.maximum(gap_min, -gap_max),
    min=0).

    One rp_trajectory_gap launch on the current stream (include/rp_batch.h: the candidates are the window's ends, the two knots and the
    roots of the relative velocity strictly inside each piece; the earliest among equal values wins; a value is bit for bit
    trajectory_eval(a, time) - trajectory_eval(b, time - delay)).  The values are differentiable to first order in all sixteen spline
    inputs, lo, hi and delay: reverse mode is one rp_trajectory_eval_vjp launch on each spline, forward mode one rp_trajectory_eval_jvp
    launch on each, at the returned times; a double backward raises torch's once_differentiable error.  At a tie
    between candidates, and where a window end is clamped, the derivative is that of the branch the forward pass found.  A NaN value has
    gradient 0 (forward mode: NaN).  The times are not differentiable.  Does not synchronise the host."""
    who = "trajectory_gap"
    _check_spline_arg("a", a, who)
    _check_spline_arg("b", b, who)
    table_a, table_b = _spline_table("a", a, who), _spline_table("b", b, who)
    _check_same_batch(table_a[0], table_b[0], who)
    lo, hi, delay = _check_gap_queries(table_a[0], lo, hi, delay, who)
    return _TrajectoryGap.apply(*table_a, *table_b, lo, hi, delay)


def _check_vehicles(pos_a, pos_b, vel_a, vel_b, who):
    """Two vehicles' problems as the min_time_* functions of two splines take them."""
    for name, pos, vel in (("pos_a", pos_a, vel_a), ("pos_b", pos_b, vel_b)):
        if not isinstance(pos, (list, tuple)) or len(pos) != 3:
            raise TypeError("%s: %s must be a list or tuple of three tensors (pos0, pos1, pos2)" % (who, name))
        if vel is not None and (not isinstance(vel, (list, tuple)) or len(vel) != 2):
            raise TypeError("%s: the velocities of %s must be None or a pair (vel0, vel2)" % (who, name))
    for name, pos in (("pos_a", pos_a), ("pos_b", pos_b)):
        _check_positions(*pos, "%s: %s" % (who, name))
    _check_same_batch(pos_a[0], pos_b[0], who)


def _solve_vehicles(pos_a, pos_b, vel_a, vel_b, gap_tol, max_iter, params):
    """min_time_solve of each (checked) vehicle: (the two splines as trajectory_gap takes them, the two solutions)."""
    splines, solutions = [], []
    for pos, vel in ((pos_a, vel_a), (pos_b, vel_b)):
        vel0, vel2 = vel if vel is not None else (None, None)
        solution = min_time_solve(*pos, gap_tol=gap_tol, max_iter=max_iter, params=params, vel0=vel0, vel2=vel2)
        splines.append(tuple(pos) + tuple(solution[:3]) + (tuple(vel) if vel is not None else ()))
        solutions.append(tuple(solution))
    return splines, solutions


def min_time_gap(pos_a, pos_b, lo=None, hi=None, delay=None, *, vel_a=None, vel_b=None, gap_tol=1e-8, max_iter=200, params=None):
    """min_time_solve of two vehicles' problems, then trajectory_gap of the two solutions.  pos_a, pos_b: (pos0, pos1, pos2) of each
    vehicle; vel_a, vel_b: (vel0, vel2) of each (None: rest to rest; either entry None: zeros); lo, hi, delay as trajectory_gap's.
    Returns (gap_min, gap_max, t_gap_min, t_gap_max, solution_a, solution_b) with each solution min_time_solve's (vel1, duration0,
    duration1, iters, status).  Plain composition: the gaps are differentiable to first order in both vehicles' positions and end
    velocities, in lo, hi and delay, in both modes, through the solves' derivatives and the gap's."""
    who = "min_time_gap"
    _check_vehicles(pos_a, pos_b, vel_a, vel_b, who)
    lo, hi, delay = _check_gap_queries(pos_a[0], lo, hi, delay, who)      # before the solves: a bad query costs none
    splines, solutions = _solve_vehicles(pos_a, pos_b, vel_a, vel_b, gap_tol, max_iter, params)
    return tuple(trajectory_gap(splines[0], splines[1], lo, hi, delay)) + (solutions[0], solutions[1])


# ---- when two splines meet: the first time the gap reaches a level ----
class _TrajectoryMeeting(torch.autograd.Function):
    """(time, relvel) of the first time in the window at which pos_A(t) - pos_B(t - delay) is at the level: time differentiable to first
    order in the sixteen spline inputs (A's table, then B's), in the level and in the delay, through the evaluator's derivative launches
    on each spline -- pos_A(theta_A, time) - pos_B(theta_B, time - delay) = level gives
    d time = (d level - d pos_A + d pos_B - vel_B d delay) / relvel.  lo and hi only choose the branch.  relvel is for the backward and is
    not differentiable."""

    @staticmethod
    def forward(*inputs):
        a, b = [_dense(t) for t in inputs[:8]], [_dense(t) for t in inputs[8:16]]
        level, lo, hi, delay = (_dense(t) for t in inputs[16:20])
        n, k = _query_shape(inputs[0].shape[0], level, lo, hi, delay)
        device = inputs[0].device
        time, relvel = _empty((n, k), device), _empty((n, k), device)
        _enqueue(capi.trajectory_meeting, device, n, k, a, b, level, lo, hi, delay, time, relvel)
        return time, relvel

    @staticmethod
    def setup_context(ctx, inputs, output):
        # neither derivative reads the level, lo or hi
        _keep(ctx, inputs, output, dead=output[1:], given=[t is not None for t in inputs[:16]] + [False, False, False, inputs[19] is not None])

    @staticmethod
    def _saved(ctx):
        """(A's and B's eight tensors; A's times, 0 where there is no meeting, and B's, those minus the delay; relvel; where there is no
        meeting)"""
        inputs, (time, relvel) = _kept(ctx)
        a, b = [_dense(t) for t in inputs[:8]], [_dense(t) for t in inputs[8:16]]
        delay = inputs[19]
        missing = torch.isnan(time)
        zero = torch.zeros_like(time)
        t_b = torch.where(missing, zero, time - delay if delay is not None else time)
        return a, b, torch.where(missing, zero, time), t_b.contiguous(), relvel, missing

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_time, _g_relvel):
        if g_time is None:
            return (None,) * 20
        a, b, t_a, t_b, relvel, missing = _TrajectoryMeeting._saved(ctx)
        need = ctx.needs_input_grad
        w = torch.where(missing, torch.zeros_like(t_a), g_time / relvel)      # an unreached level: gradient 0
        bars = _bars(need[:16], t_a.shape[0], t_a.device)
        tau_bar = _empty(t_a.shape, t_a.device) if need[19] else None
        if any(x is not None for x in bars[:8]):
            _enqueue(capi.trajectory_eval_vjp, t_a.device, *t_a.shape, a, t_a, -w, None, None, bars[:8], None)
        if tau_bar is not None or any(x is not None for x in bars[8:]):      # B is at time - delay
            _enqueue(capi.trajectory_eval_vjp, t_a.device, *t_a.shape, b, t_b, w, None, None, bars[8:], tau_bar)
        return tuple(bars) + (w if need[16] else None, None, None, -tau_bar if tau_bar is not None else None)

    @staticmethod
    def jvp(ctx, *tangents):
        a, b, t_a, t_b, relvel, missing = _TrajectoryMeeting._saved(ctx)
        dots = [_dense(t) for t in tangents[:16]]
        level_dot, delay_dot = tangents[16], tangents[19]
        pos_a, pos_b = _empty(t_a.shape, t_a.device), _empty(t_a.shape, t_a.device)
        _enqueue(capi.trajectory_eval_jvp, t_a.device, *t_a.shape, a, t_a, dots[:8], None, pos_a, None, None)
        _enqueue(capi.trajectory_eval_jvp, t_a.device, *t_a.shape, b, t_b, dots[8:], (-delay_dot).contiguous() if delay_dot is not None else None,
                 pos_b, None, None)
        if level_dot is None:
            level_dot = torch.zeros_like(t_a)
        time_dot = torch.where(missing, torch.full_like(t_a, float("nan")), (level_dot - pos_a + pos_b) / relvel)
        return time_dot, None


def _check_meeting_queries(pos0, level, lo, hi, delay, who):
    """level (None: 0), lo, hi (None: -inf / +inf) and delay (None: 0)."""
    return _check_named_queries(pos0, (("level", level), ("lo", lo), ("hi", hi), ("delay", delay)), who)


def trajectory_meeting(a, b, level=None, lo=None, hi=None, delay=None):
    """The first time at which the gap between two splines of trajectory_eval in one frame, D(t) = pos_a(t) - pos_b(t - delay), is at
    `level`, within the windows of time [lo, hi]: the inverse of trajectory_gap's D as trajectory_crossing is of trajectory_eval's pos.
    a, b, lo, hi, delay: exactly trajectory_gap's; level: (n, k) or (k,) like them; None: 0, the two vehicles at the same position; all
    four None: k = 1, the whole common domain.  Returns the times (on a's clock), (n, k): NaN where the gap does not reach the level in the
    window clamped to [max(delay, 0), min(T_a, delay + T_b)] (no extrapolation), where the clamped window is empty, where the level is NaN
    or infinite or the delay NaN or infinite, and for a problem either of whose splines has a duration that is not finite or not > 0.

    One rp_trajectory_meeting launch on the current stream (include/rp_batch.h: the first of the gap's nine monotone sub-pieces that holds
    the level, then trajectory_crossing's bracketed Newton search with its fixed trip bound; a level within rounding of an extreme of D
    may give the touch, a later meeting, or NaN).  Differentiable to first order in all sixteen spline inputs, the level and the delay,
    d time = (d level - d pos_a + d pos_b - vel_b d delay) / relvel with relvel the closing velocity D'(time): reverse mode is one
    rp_trajectory_eval_vjp launch on each spline, forward mode one rp_trajectory_eval_jvp launch on each; a double
    backward raises torch's once_differentiable error.  lo and hi get no gradient: the time depends on them through the branch only --
    a time that sits on the window's start because D is at the level there still moves with the level, not with lo.  An unreached level
    has gradient 0 (forward mode: NaN, as the time); where the closing velocity is 0 (a touch) there is no derivative and the result is inf
    or NaN; the time jumps where an earlier extreme of D passes through the level.  Does not synchronise the host."""
    who = "trajectory_meeting"
    _check_spline_arg("a", a, who)
    _check_spline_arg("b", b, who)
    table_a, table_b = _spline_table("a", a, who), _spline_table("b", b, who)
    _check_same_batch(table_a[0], table_b[0], who)
    level, lo, hi, delay = _check_meeting_queries(table_a[0], level, lo, hi, delay, who)
    return _TrajectoryMeeting.apply(*table_a, *table_b, level, lo, hi, delay)[0]


def min_time_meeting(pos_a, pos_b, level=None, lo=None, hi=None, delay=None, *, vel_a=None, vel_b=None, gap_tol=1e-8, max_iter=200,
                     params=None):
    """min_time_solve of two vehicles' problems, then trajectory_meeting of the two solutions.  pos_a, pos_b, vel_a, vel_b as
    min_time_gap's; level, lo, hi, delay as trajectory_meeting's.  Returns (time, solution_a, solution_b) with each solution
    min_time_solve's (vel1, duration0, duration1, iters, status).  Plain composition: the times are differentiable to first order in both
    vehicles' positions and end velocities, in the level and the delay, in both modes, through the solves' derivatives and the meeting's."""
    who = "min_time_meeting"
    _check_vehicles(pos_a, pos_b, vel_a, vel_b, who)
    level, lo, hi, delay = _check_meeting_queries(pos_a[0], level, lo, hi, delay, who)      # before the solves: a bad query costs none
    splines, solutions = _solve_vehicles(pos_a, pos_b, vel_a, vel_b, gap_tol, max_iter, params)
    return trajectory_meeting(splines[0], splines[1], level, lo, hi, delay), solutions[0], solutions[1]


# ---- how close two vehicles moving in several axes get: the least squared distance over a window ----
class _TrajectorySeparation(torch.autograd.Function):
    """(sep_sq, t_closest) of two vehicles of d axes over the windows [lo, hi] clamped to the 2 d splines' common domain.  Inputs: d, then
    A's 8 d tensors (axis-major, each axis in the table's order), B's 8 d, then lo, hi, delay.  The value is differentiable to first order
    in all 16 d spline inputs, lo, hi and the delay by the envelope theorem: per axis one launch of the evaluator's derivative on A_c at
    the returned time with 2 g D_c and one on B_c at time - delay with -2 g D_c, the time's own derivative routed by the class of the time
    -- lo, hi, the end of an A_c, the end of a B_c, the delayed start; dropped at a stationary point, a knot or the clamp +0.0 (DESIGN.md
    section 24).  The time is not differentiable."""

    @staticmethod
    def forward(d, *inputs):
        a, b = [_dense(t) for t in inputs[:8 * d]], [_dense(t) for t in inputs[8 * d:16 * d]]
        lo, hi, delay = (_dense(t) for t in inputs[16 * d:])
        n, k = _query_shape(inputs[0].shape[0], lo, hi, delay)
        device = inputs[0].device
        value, time = _empty((n, k), device), _empty((n, k), device)
        _enqueue(capi.trajectory_separation, device, n, k, d, a, b, lo, hi, delay, value, time)
        return value, time

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.d = inputs[0]
        _keep(ctx, inputs[1:], output, dead=output[1:])

    @staticmethod
    def _saved(ctx):
        """(A's and B's d lists of eight tensors; the delay (zeros for None); the time, 0 where the value is NaN, and B's, that minus the
        delay; where it is NaN; the d gaps D_c there; the class masks LO, HI, [END of A_c], [END of B_c], START, exclusive and in that
        priority)"""
        d = ctx.d
        inputs, (value, time) = _kept(ctx)
        a, b = _axis_tables(inputs, d)
        lo, hi, delay = inputs[16 * d:]
        missing = torch.isnan(value) | torch.isnan(time)
        zero = torch.zeros_like(time)
        t_a = torch.where(missing, zero, time).contiguous()
        shift = delay if delay is not None else zero
        t_b = torch.where(missing, zero, t_a - shift).contiguous()
        tests = [lo, hi] + [(s[6] + s[7]).unsqueeze(1) for s in a] + [shift + (s[6] + s[7]).unsqueeze(1) for s in b] + [shift]
        masks = _class_masks(t_a, missing, tests, last_only=shift > 0)      # a start clamped to +0.0 is a constant
        return a, b, shift, t_a, t_b, missing, _pair_gaps(a, b, t_a, t_b), (masks[0], masks[1], masks[2:2 + d], masks[2 + d:2 + 2 * d], masks[-1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_value, _g_time):
        d = ctx.d
        if g_value is None:
            return (None,) * (16 * d + 4)
        a, b, _, t_a, t_b, missing, gaps, (is_lo, is_hi, end_a, end_b, start) = _TrajectorySeparation._saved(ctx)
        n = t_a.shape[0]
        g = torch.where(missing, torch.zeros_like(g_value), g_value)      # a NaN value: gradient 0
        need = ctx.needs_input_grad[1:]
        want_time = any(need[8 * c + 6] or need[8 * c + 7] for c in range(2 * d)) or any(need[16 * d:])
        bars, time_bar, shift_bar = [None] * (16 * d), None, None
        for c in range(d):
            g_pos = ((2.0 * g) * gaps[c]).contiguous()
            for side, spline, tau, upstream in ((0, a[c], t_a, g_pos), (1, b[c], t_b, -g_pos)):
                first = 8 * (side * d + c)
                bar = _bars(need[first:first + 8], n, tau.device)
                tau_bar = _empty(tau.shape, tau.device) if want_time else None
                if want_time or any(x is not None for x in bar):
                    _enqueue(capi.trajectory_eval_vjp, tau.device, *tau.shape, spline, tau, upstream, None, None, bar, tau_bar)
                bars[first:first + 8] = bar
                if want_time:
                    time_bar = tau_bar if time_bar is None else time_bar + tau_bar
                    if side:
                        shift_bar = tau_bar if shift_bar is None else shift_bar + tau_bar
        lo_bar = hi_bar = delay_bar = None
        if want_time:
            routed = lambda mask: torch.where(mask, time_bar, torch.zeros_like(time_bar))      # noqa: E731
            for side, ends in ((0, end_a), (1, end_b)):
                for c in range(d):
                    for f in (6, 7):
                        at = 8 * (side * d + c) + f
                        if need[at]:
                            bars[at] = bars[at] + routed(ends[c]).sum(dim=1)
            if need[16 * d]:
                lo_bar = routed(is_lo)
            if need[16 * d + 1]:
                hi_bar = routed(is_hi)
            if need[16 * d + 2]:      # B is at time - delay, and the times that hold the delay move with it
                holds = start
                for mask in end_b:
                    holds = holds | mask
                delay_bar = routed(holds) - shift_bar
        return (None,) + tuple(bars) + (lo_bar, hi_bar, delay_bar)

    @staticmethod
    def jvp(ctx, _t_d, *tangents):
        d = ctx.d
        a, b, _, t_a, t_b, missing, gaps, (is_lo, is_hi, end_a, end_b, start) = _TrajectorySeparation._saved(ctx)
        n, k = t_a.shape
        dots = [_dense(t) for t in tangents[:16 * d]]
        zero = torch.zeros_like(t_a)
        col = lambda t: t.unsqueeze(1).expand(n, k) if t is not None else zero      # noqa: E731
        wide = lambda t: t if t is not None else zero      # noqa: E731
        delay_dot = wide(tangents[16 * d + 2])
        time_dot = torch.where(is_lo, wide(tangents[16 * d]), zero)
        time_dot = torch.where(is_hi, wide(tangents[16 * d + 1]), time_dot)
        for c in range(d):
            time_dot = torch.where(end_a[c], col(dots[8 * c + 6]) + col(dots[8 * c + 7]), time_dot)
            time_dot = torch.where(end_b[c], delay_dot + col(dots[8 * (d + c) + 6]) + col(dots[8 * (d + c) + 7]), time_dot)
        time_dot = torch.where(start, delay_dot, time_dot)
        value_dot = zero
        for c in range(d):
            pos_a, pos_b = _empty(t_a.shape, t_a.device), _empty(t_a.shape, t_a.device)
            _enqueue(capi.trajectory_eval_jvp, t_a.device, n, k, a[c], t_a, dots[8 * c:8 * c + 8], time_dot.contiguous(), pos_a, None, None)
            _enqueue(capi.trajectory_eval_jvp, t_a.device, n, k, b[c], t_b, dots[8 * (d + c):8 * (d + c) + 8],
                     (time_dot - delay_dot).contiguous(), pos_b, None, None)
            value_dot = value_dot + (2.0 * gaps[c]) * (pos_a - pos_b)
        return torch.where(missing, torch.full_like(t_a, float("nan")), value_dot), None


def _check_axes(name, spline, who):
    """One vehicle's (checked) sequence of six or eight tensors, (n, d) or (n,) each: d, and the d splines as _spline_table takes them."""
    pos0 = spline[0]
    _check_is_tensor(name + ": pos0", pos0, who)
    if pos0.dim() not in (1, 2):
        raise ValueError("%s: %s: pos0 must have shape (n, d) or (n,), got %s" % (who, name, tuple(pos0.shape)))
    d = pos0.shape[1] if pos0.dim() == 2 else 1
    if not 1 <= d <= 3:
        raise ValueError("%s: %s has %d axes; one, two or three are supported" % (who, name, d))
    for t in spline[1:]:
        if t is None:
            continue
        _check_is_tensor(name, t, who)
        if t.shape != pos0.shape:
            raise ValueError("%s: %s: a tensor has shape %s, pos0 %s" % (who, name, tuple(t.shape), tuple(pos0.shape)))
    if pos0.dim() == 1:
        return 1, [list(spline)]
    return d, [[t[:, c] if t is not None else None for t in spline] for c in range(d)]


def trajectory_separation(a, b, lo=None, hi=None, delay=None):
    """The closest approach of two vehicles that move in d = 1, 2 or 3 axes, each axis a spline of trajectory_eval solved on its own: the
    least squared distance f(t) = sum over the axes of (pos_a,c(t) - pos_b,c(t - delay))^2 over the windows of time [lo, hi], and when it
    is attained.  a, b: each a sequence of six tensors (pos0, pos1, pos2, vel1, duration0, duration1), or of eight with (vel0, vel2)
    appended, each (n, d), or (n,) for d = 1, on the same ROCm device.  lo, hi, delay: (n, k), or (k,) for the same queries in every
    problem; None: -inf / +inf / 0, all three None: k = 1, the whole common domain.  b's clock starts `delay` after a's, one delay for all
    axes; no extrapolation: the window is clamped to [max(delay, 0), the smallest of the 2 d ends T_a,c and delay + T_b,c] -- with axes of
    different total times the domain ends when the fastest axis does (synchronize_axes stretches them to the slowest).  Returns (sep_sq,
    t_closest), (n, k) each; the distance is sep_sq.sqrt().  NaN where the clamped window is empty, where the delay is NaN or infinite, and
    for a problem any of whose 2 d splines has a duration that is not finite or not > 0.

    One rp_trajectory_separation launch on the current stream (include/rp_batch.h: the candidates are the window's ends, the knots and
    the stationary points of f on each piece between knots, the real roots of a quintic; the earliest among equal values wins; a value is
    bit for bit the sum in axis order of the squares of trajectory_eval(a_c, time) - trajectory_eval(b_c, time - delay)).  sep_sq is
    differentiable to first order in all 16 d spline inputs, lo, hi and delay by the envelope theorem: per axis one rp_trajectory_eval
    launch and one rp_trajectory_eval_vjp (reverse mode) or rp_trajectory_eval_jvp (forward mode) launch on each spline at the returned
    time; a double backward raises torch's once_differentiable error.  At a tie between candidates, and where a
    window end is clamped, the derivative is that of the branch the forward pass found.  A NaN value has gradient 0 (forward mode: NaN).
    The time is not differentiable.  Does not synchronise the host."""
    who = "trajectory_separation"
    _check_spline_arg("a", a, who)
    _check_spline_arg("b", b, who)
    d, axes_a = _check_axes("a", a, who)
    d_b, axes_b = _check_axes("b", b, who)
    if d_b != d:
        raise ValueError("%s: a has %d axes, b %d" % (who, d, d_b))
    tables_a = [_spline_table("a, axis %d" % c, s, who) for c, s in enumerate(axes_a)]
    tables_b = [_spline_table("b, axis %d" % c, s, who) for c, s in enumerate(axes_b)]
    _check_same_batch(tables_a[0][0], tables_b[0][0], who)
    lo, hi, delay = _check_gap_queries(tables_a[0][0], lo, hi, delay, who)
    flat = [t for table in tables_a + tables_b for t in table]
    return _TrajectorySeparation.apply(d, *flat, lo, hi, delay)


def synchronize_axes(spline):
    """A rest-to-rest vehicle's axes stretched in time to its slowest: spline is six tensors (pos0, pos1, pos2, vel1, duration0,
    duration1), (n, d) each; with T_c = duration0 + duration1 of axis c and s = max_c T_c / T_c >= 1, the durations are multiplied by s
    and vel1 is divided by it.  Every axis then runs through the same positions at s times the time -- the path is the same, the
    velocities are divided by s and the accelerations by s^2, so the limits of the solve still hold -- and all axes end together.  Returns
    (the stretched six tensors, s).  Plain torch: differentiable, on any device."""
    if not isinstance(spline, (list, tuple)) or len(spline) != 6:
        raise TypeError("synchronize_axes: spline must be a list or tuple of six tensors (pos0, pos1, pos2, vel1, duration0, duration1)")
    pos0, pos1, pos2, vel1, duration0, duration1 = spline
    for name, t in zip(("pos0", "pos1", "pos2", "vel1", "duration0", "duration1"), spline):
        _check_is_tensor(name, t, "synchronize_axes")
        if t.dim() != 2 or t.shape != pos0.shape:
            raise ValueError("synchronize_axes: %s must have pos0's shape (n, d), got %s" % (name, tuple(t.shape)))
    total = duration0 + duration1
    s = total.max(dim=1, keepdim=True).values / total
    return [pos0, pos1, pos2, vel1 / s, duration0 * s, duration1 * s], s


def _check_axis_vehicles(pos_a, pos_b, vel_a, vel_b, synchronize, who):
    """Two vehicles of d axes as min_time_separation and min_time_contact take them: per vehicle (its three positions, its end velocities or
    None), each (n, d) tensor flattened axis-major to n d problems."""
    if synchronize and (vel_a is not None or vel_b is not None):
        raise ValueError(who + ": synchronize=True needs rest-to-rest vehicles; pass synchronize=False with end velocities")
    flat = []
    for name, pos, vel in (("pos_a", pos_a, vel_a), ("pos_b", pos_b, vel_b)):
        if not isinstance(pos, (list, tuple)) or len(pos) != 3:
            raise TypeError("%s: %s must be a list or tuple of three tensors (pos0, pos1, pos2)" % (who, name))
        if vel is not None and (not isinstance(vel, (list, tuple)) or len(vel) != 2):
            raise TypeError("%s: the velocities of %s must be None or a pair (vel0, vel2)" % (who, name))
        for t in list(pos) + [v for v in (vel or ()) if v is not None]:
            _check_is_tensor(name, t, who)
            if t.dim() != 2 or t.shape != pos[0].shape or not 1 <= t.shape[1] <= 3:
                raise ValueError("%s: every tensor of %s must have one shape (n, d) with d in 1..3, got %s" % (who, name, tuple(t.shape)))
        flat.append(([t.t().reshape(-1) for t in pos], [v.t().reshape(-1) if v is not None else None for v in vel] if vel is not None else None))
    if pos_a[0].shape != pos_b[0].shape:
        raise ValueError("%s: pos_a has shape %s, pos_b %s" % (who, tuple(pos_a[0].shape), tuple(pos_b[0].shape)))
    _check_vehicles(flat[0][0], flat[1][0], flat[0][1], flat[1][1], who)
    return flat


def _solve_axis_vehicles(pos_a, pos_b, flat, synchronize, gap_tol, max_iter, params):
    """min_time_solve of each (checked) vehicle over its n d axis problems: (the two vehicles as trajectory_separation takes them, stretched
    to their slowest axes if asked; the two solutions as (n, d), as the solve left them)."""
    n, d = pos_a[0].shape
    splines, solutions = [], []
    for pos, (flat_pos, flat_vel) in zip((pos_a, pos_b), flat):
        vel0, vel2 = flat_vel if flat_vel is not None else (None, None)
        solution = min_time_solve(*flat_pos, gap_tol=gap_tol, max_iter=max_iter, params=params, vel0=vel0, vel2=vel2)
        solution = tuple(t.reshape(d, n).t() for t in solution)
        spline = list(pos) + list(solution[:3])
        if synchronize:
            spline, _ = synchronize_axes(spline)
        elif flat_vel is not None:
            spline = spline + [v.reshape(d, n).t() if v is not None else None for v in flat_vel]
        splines.append(spline)
        solutions.append(solution)
    return splines, solutions


def min_time_separation(pos_a, pos_b, lo=None, hi=None, delay=None, *, vel_a=None, vel_b=None, synchronize=True, gap_tol=1e-8, max_iter=200,
                        params=None):
    """min_time_solve of two vehicles' axes, then trajectory_separation of the two solutions.  pos_a, pos_b: (pos0, pos1, pos2) of each
    vehicle, (n, d) each; each vehicle is one solve over its n d axis problems.  vel_a, vel_b: (vel0, vel2) of each, (n, d) (None: rest to
    rest).  synchronize (the default): each vehicle's axes are stretched to its slowest first (synchronize_axes; rest to rest only: with
    end velocities given it raises ValueError).  lo, hi, delay as trajectory_separation's.  Returns (sep_sq, t_closest, solution_a,
    solution_b) with each solution min_time_solve's (vel1, duration0, duration1, iters, status) as (n, d), as the solve left them (before
    the stretch).  Plain composition: sep_sq is differentiable to first order in both vehicles' positions and end velocities, in lo, hi
    and delay, in both modes."""
    who = "min_time_separation"
    flat = _check_axis_vehicles(pos_a, pos_b, vel_a, vel_b, synchronize, who)
    if any(x is not None for x in (lo, hi, delay)):      # before the solves: a bad query costs none
        lo, hi, delay = _check_gap_queries(pos_a[0][:, 0], lo, hi, delay, who)
    splines, solutions = _solve_axis_vehicles(pos_a, pos_b, flat, synchronize, gap_tol, max_iter, params)
    return tuple(trajectory_separation(splines[0], splines[1], lo, hi, delay)) + (solutions[0], solutions[1])


# ---- the closest approach of every pair of a fleet ----
FLEET_MOST = 256      # vehicles per scene (csrc/fleet_index.h)
CROSS_MOST = 32768    # vehicles per scene and fleet of the cross queries (csrc/fleet_index.h)


def _check_fleet_size(m, who):
    if isinstance(m, bool) or not isinstance(m, int):
        raise TypeError("%s: m must be an int, got %s" % (who, type(m).__name__))
    if not 2 <= m <= FLEET_MOST:
        raise ValueError("%s: a scene holds 2..%d vehicles, got m = %d" % (who, FLEET_MOST, m))


def fleet_pairs(m, device=None):
    """The pairs (i, j), i < j, of m vehicles (2..256) in the order of trajectory_fleet_separation's outputs -- lexicographic,
    torch.triu_indices(m, m, 1)'s: a (m (m - 1) / 2, 2) int64 tensor on `device`."""
    _check_fleet_size(m, "fleet_pairs")
    return torch.triu_indices(m, m, 1, device=device).t().contiguous()


@functools.lru_cache(maxsize=64)
def _fleet_slots_cpu(m):
    first, second = torch.triu_indices(m, m, 1)
    pair_at = torch.zeros((m, m), dtype=torch.int64)
    pair_at[first, second] = torch.arange(first.shape[0])
    pair_at = pair_at + pair_at.t()
    vehicle = torch.arange(m).unsqueeze(1)
    partner = torch.arange(m - 1).unsqueeze(0) + (torch.arange(m - 1).unsqueeze(0) >= vehicle)      # every other vehicle, increasing
    sign = torch.where(vehicle < partner, 1.0, -1.0).to(torch.float64)
    return pair_at.gather(1, partner), sign, partner


@functools.lru_cache(maxsize=64)
def _fleet_slots_on(m, device):
    pair, sign, _ = _fleet_slots_cpu(m)
    first, second = torch.triu_indices(m, m, 1)
    # where a pair's two entries lie in the (m, m - 1) table, flattened: vehicle i's row holds partner j > i at j - 1, vehicle j's holds i at i
    return (pair.to(device), sign.to(device), (first * (m - 1) + second - 1).to(device), (second * (m - 1) + first).to(device),
            first.to(device), second.to(device))


def fleet_slots(m, device=None):
    """The inverse of fleet_pairs as the derivative routing uses it: (pair, sign, partner), (m, m - 1) each -- vehicle v's row lists the
    pairs that contain it (indices into fleet_pairs(m)), partners in increasing order, with +1.0 where v is the pair's first vehicle
    and -1.0 where it is the second.  Every sum over a vehicle's pairs is a gather through this table and a sum: no atomics."""
    _check_fleet_size(m, "fleet_slots")
    return tuple(t.to(device) if device is not None else t.clone() for t in _fleet_slots_cpu(m))


# What the four fleet Functions share: one forward launch each; for the derivatives the pair entry's rule done per
# vehicle -- the times gathered through the slot table to (n m, (m - 1) k), per axis one evaluator launch and one launch of its derivative
# on the n m splines, every sum over a vehicle's pairs a gather through the slot table and a sum.
def _fleet_forward(entry, d, m, inputs, n, k, outputs, *middle, tail=()):
    """One launch of a fleet entry on the current stream: the fleet's 8 d tensors (inputs[:8 d]; axis-major, each axis in the table's
    order, each n m values with vehicle v of scene s at s m + v), `middle`, then `outputs` fresh (n, pairs, k) tensors, which it returns,
    then `tail`."""
    sizes, pairs = (m, m[0] * m[1]) if isinstance(m, tuple) else ((m,), m * (m - 1) // 2)      # (m_a, m_b): a cross entry, two tables
    fleets = [[_dense(t) for t in inputs[8 * d * v:8 * d * (v + 1)]] for v in range(len(sizes))]
    out = tuple(_empty((n, pairs, k), inputs[0].device) for _ in range(outputs))
    _enqueue(entry, inputs[0].device, n, *sizes, k, d, *fleets, *middle, *out, *tail)
    return out


def _fleet_setup(ctx, inputs, count, dead, outputs):
    """Keeps d, m, those of the first `count` inputs after them that were given, and `outputs`, for both modes (_keep); `dead` are the
    outputs that are not differentiable."""
    ctx.d, ctx.m = inputs[0], inputs[1]
    _keep(ctx, inputs[2:2 + count], outputs, dead)


def _fleet_kept(ctx):
    """What _fleet_setup kept: (the d lists of eight fleet tensors, the other inputs among the `count`, the outputs)"""
    inputs, outputs = _kept(ctx)
    return _axis_tables(inputs, ctx.d, 1)[0], inputs[8 * ctx.d:], outputs


_FleetTimes = collections.namedtuple("_FleetTimes", "slots signs delay t tau per_pair through")


def _fleet_times(m, time, missing, start=None):
    """Where the derivatives evaluate the n m splines.  time: each pair's time on the clock of its first vehicle, (n, pairs, k).  Returns
    slots: the slot tables; signs: +1 / -1 as (1, m, m - 1, 1); delay: start_j - start_i, (n, pairs, 1), the kernel's bits (None without
    start); t: the time, 0 where missing; tau: the times through the slot table, (n m, (m - 1) k) -- t in both vehicles' rows or, with
    start, t in the row of the pair's first vehicle and t - delay, the pair entry's t_b, in the row of its second;
    per_pair: a pair's view of a per-slot array; through: (n, pairs, k) -> per vehicle and slot, (n, m, m - 1, k)."""
    n, pairs, k = time.shape
    slots = _fleet_slots_on(m, time.device)
    pair, sign, at_first, at_second, first, second = slots
    through = lambda x: x[:, pair.reshape(-1), :].reshape(n, m, m - 1, k)      # noqa: E731
    signs = sign.reshape(1, m, m - 1, 1)
    zero = torch.zeros_like(time)
    t = torch.where(missing, zero, time)
    if start is None:
        delay, rows = None, through(t)
    else:
        delay = (start[:, second] - start[:, first]).unsqueeze(2)
        rows = torch.where(signs > 0, through(t), through(torch.where(missing, zero, t - delay)))
    tau = rows.reshape(n * m, (m - 1) * k).contiguous()

    def per_pair(x):      # (n m, (m - 1) k) -> the pair's entry in its first vehicle's row and in its second's, (n, pairs, k) each
        x = x.reshape(n, m * (m - 1), k)
        return x[:, at_first, :], x[:, at_second, :]

    return _FleetTimes(slots, signs, delay, t, tau, per_pair, through)


def _fleet_gaps(fleet, at):
    """The d gaps D_c at the pairs' times, (n, pairs, k) each: one evaluator launch per axis"""
    gaps = []
    for s in fleet:
        pos = _empty(at.tau.shape, at.tau.device)
        _enqueue(capi.trajectory_eval, at.tau.device, *at.tau.shape, s, at.tau, pos, None, None)
        pos_first, pos_second = at.per_pair(pos)
        gaps.append(pos_first - pos_second)
    return gaps


def _fleet_vjp(fleet, at, need, want_tau, g_gap):
    """Axis by axis, the evaluator's reverse launch on the n m splines at at.tau, upstream g_gap(c) -- the gradient on the gap D_c,
    (n, pairs, k) -- with its sign through the slot table; yields (the axis' eight bars, None where need has none; tau_bar, None unless
    want_tau).  An axis that needs neither is not launched."""
    tau = at.tau
    for c, s in enumerate(fleet):
        bar = _bars(need[8 * c:8 * c + 8], tau.shape[0], tau.device)
        tau_bar = _empty(tau.shape, tau.device) if want_tau else None
        if want_tau or any(x is not None for x in bar):
            upstream = (at.signs * at.through(g_gap(c))).reshape(tau.shape).contiguous()
            _enqueue(capi.trajectory_eval_vjp, tau.device, *tau.shape, s, tau, upstream, None, None, bar, tau_bar)
        yield bar, tau_bar


def _fleet_jvp(fleet, at, gaps, dots, tau_dot):
    """Axis by axis, the evaluator's forward launch on the n m splines at at.tau; yields the axis' share of the tangent of the squared
    distance, 2 D_c (d pos_first,c - d pos_second,c), (n, pairs, k)."""
    for c, s in enumerate(fleet):
        pos_dot = _empty(at.tau.shape, at.tau.device)
        _enqueue(capi.trajectory_eval_jvp, at.tau.device, *at.tau.shape, s, at.tau, dots[8 * c:8 * c + 8], tau_dot, pos_dot, None, None)
        dot_first, dot_second = at.per_pair(pos_dot)
        yield (2.0 * gaps[c]) * (dot_first - dot_second)


def _route_end_bars(bars, need, at, routed, end_first, end_second):
    """Adds to the duration bars what the times that sit on a vehicle's end carry: a vehicle's pairs through the slot table, then a
    plain sum."""
    for c in range(len(end_first)):
        if need[8 * c + 6] or need[8 * c + 7]:
            mine = torch.where(at.signs > 0, at.through(routed(end_first[c])), at.through(routed(end_second[c]))).sum(dim=(2, 3)).reshape(-1)
            for f in (6, 7):
                if need[8 * c + f]:
                    bars[8 * c + f] = bars[8 * c + f] + mine


class _TrajectoryFleetSeparation(torch.autograd.Function):
    """(sep_sq, t_closest), (n, pairs, k) each, of every pair of n scenes of m vehicles of d axes over the scenes' windows.  Inputs: d, m,
    the fleet's 8 d tensors, lo, hi (n, k).  The value is differentiable to first order in all 8 d fleet inputs, lo and hi by
    _TrajectorySeparation's envelope routing done per vehicle, the time's own derivative routed by the class of the time -- lo, hi, the
    end of an axis of the pair's first vehicle, of its second; dropped otherwise.  The time is not differentiable."""

    @staticmethod
    def forward(d, m, *inputs):
        lo, hi = (_dense(t) for t in inputs[8 * d:])
        given = lo if lo is not None else hi
        n = inputs[0].shape[0] // m
        k = given.shape[1] if given is not None else 1
        return _fleet_forward(capi.trajectory_fleet_separation, d, m, inputs, n, k, 2, lo, hi)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _fleet_setup(ctx, inputs, 8 * inputs[0] + 2, output[1:], output)

    @staticmethod
    def _saved(ctx):
        """(the d lists of eight tensors; _fleet_times; where the value is NaN, (n, pairs, k); the d gaps D_c; the class masks LO, HI,
        [END of the first vehicle's axis c], [END of the second's], exclusive and in that priority)"""
        d, m = ctx.d, ctx.m
        fleet, (lo, hi), (value, time) = _fleet_kept(ctx)
        missing = torch.isnan(value) | torch.isnan(time)
        at = _fleet_times(m, time, missing)
        first, second = at.slots[4], at.slots[5]
        ends = [(s[6] + s[7]).reshape(-1, m) for s in fleet]
        tests = [lo.unsqueeze(1) if lo is not None else None, hi.unsqueeze(1) if hi is not None else None]
        tests += [e[:, first].unsqueeze(2) for e in ends] + [e[:, second].unsqueeze(2) for e in ends]
        masks = _class_masks(at.t, missing, tests)
        return fleet, at, missing, _fleet_gaps(fleet, at), (masks[0], masks[1], masks[2:2 + d], masks[2 + d:])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_value, _g_time):
        d = ctx.d
        if g_value is None:
            return (None,) * (8 * d + 4)
        fleet, at, missing, gaps, (is_lo, is_hi, end_first, end_second) = _TrajectoryFleetSeparation._saved(ctx)
        g = torch.where(missing, torch.zeros_like(g_value), g_value)      # a NaN value: gradient 0
        need = ctx.needs_input_grad[2:]
        want_time = any(need[8 * c + 6] or need[8 * c + 7] for c in range(d)) or any(need[8 * d:])
        # (a bad vehicle's gap is NaN: not into its partners)
        g_gap = lambda c: torch.where(missing, torch.zeros_like(g), (2.0 * g) * gaps[c])      # noqa: E731
        bars, time_bar = [], None
        for bar, tau_bar in _fleet_vjp(fleet, at, need, want_time, g_gap):
            bars += bar
            if want_time:      # the pair's: its two vehicles', added in _TrajectorySeparation's order -- the same bits per pair and query
                for share in at.per_pair(tau_bar):
                    time_bar = share if time_bar is None else time_bar + share
        lo_bar = hi_bar = None
        if want_time:
            routed = lambda mask: torch.where(mask, time_bar, torch.zeros_like(time_bar))      # noqa: E731
            _route_end_bars(bars, need, at, routed, end_first, end_second)
            if need[8 * d]:
                lo_bar = routed(is_lo).sum(dim=1)
            if need[8 * d + 1]:
                hi_bar = routed(is_hi).sum(dim=1)
        return (None, None) + tuple(bars) + (lo_bar, hi_bar)

    @staticmethod
    def jvp(ctx, _t_d, _t_m, *tangents):
        d, m = ctx.d, ctx.m
        fleet, at, missing, gaps, (is_lo, is_hi, end_first, end_second) = _TrajectoryFleetSeparation._saved(ctx)
        pair, first, second = at.slots[0], at.slots[4], at.slots[5]
        dots = [_dense(t) for t in tangents[:8 * d]]
        zero = torch.zeros(missing.shape, dtype=torch.float64, device=at.tau.device)
        wide = lambda t: t.unsqueeze(1) if t is not None else zero      # noqa: E731
        time_dot = torch.where(is_lo, wide(tangents[8 * d]), zero)
        time_dot = torch.where(is_hi, wide(tangents[8 * d + 1]), time_dot)
        for which, ends in ((first, end_first), (second, end_second)):
            for c in range(d):
                total = None
                for t in (dots[8 * c + 6], dots[8 * c + 7]):
                    if t is not None:
                        total = t if total is None else total + t
                if total is not None:
                    time_dot = torch.where(ends[c], total.reshape(-1, m)[:, which].unsqueeze(2), time_dot)
        tau_dot = time_dot[:, pair.reshape(-1), :].reshape(at.tau.shape).contiguous()
        value_dot = zero
        for share in _fleet_jvp(fleet, at, gaps, dots, tau_dot):
            value_dot = value_dot + share
        return torch.where(missing, torch.full_like(zero, float("nan")), value_dot), None


class _TrajectoryStaggeredSeparation(torch.autograd.Function):
    """_TrajectoryFleetSeparation with a start time per vehicle: (sep_sq, t_closest on the scene's clock, t_closest on the clock of the pair's
    first vehicle), (n, pairs, k) each.  Inputs: d, m, the fleet's 8 d tensors, start (n, m), lo, hi (n, k).  Pair (i, j) is
    _TrajectorySeparation's query with delay = start_j - start_i over [lo - start_i, hi - start_i], and so are its derivatives: vehicle i
    is evaluated at the local time t', vehicle j at t' - delay, the classes are tested on t' in that function's priority -- LO, HI, the
    END of an axis of the first vehicle, of the second (delay + T), the delayed START --, delay_bar = routed(END of the second | START) -
    the sum of the second vehicle's tau_bar, and start_j gets delay_bar, start_i minus (delay_bar + the pair's lo_bar + hi_bar): every sum
    over pairs a gather through the slot table and a sum.  The times are not differentiable."""

    @staticmethod
    def forward(d, m, *inputs):
        start, lo, hi = (_dense(t) for t in inputs[8 * d:])
        given = lo if lo is not None else hi
        n = start.shape[0]
        k = given.shape[1] if given is not None else 1
        return _fleet_forward(capi.trajectory_fleet_separation_staggered, d, m, inputs, n, k, 3, start, lo, hi)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _fleet_setup(ctx, inputs, 8 * inputs[0] + 3, output[1:], (output[0], output[2]))

    @staticmethod
    def _saved(ctx):
        """_TrajectoryFleetSeparation._saved's, the times the local ones, with the class mask START after the others"""
        d, m = ctx.d, ctx.m
        fleet, (start, lo, hi), (value, local) = _fleet_kept(ctx)
        missing = torch.isnan(value) | torch.isnan(local)
        at = _fleet_times(m, local, missing, start)
        first, second = at.slots[4], at.slots[5]
        s_first = start[:, first].unsqueeze(2)
        ends = [(s[6] + s[7]).reshape(-1, m) for s in fleet]
        tests = [lo.unsqueeze(1) - s_first if lo is not None else None, hi.unsqueeze(1) - s_first if hi is not None else None]
        tests += [e[:, first].unsqueeze(2) for e in ends] + [at.delay + e[:, second].unsqueeze(2) for e in ends] + [at.delay]
        masks = _class_masks(at.t, missing, tests, at.delay > 0)      # a start clamped to +0.0 is a constant
        return fleet, at, missing, _fleet_gaps(fleet, at), (masks[0], masks[1], masks[2:2 + d], masks[2 + d:2 + 2 * d], masks[-1])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_value, _g_time, _g_local):
        d = ctx.d
        if g_value is None:
            return (None,) * (8 * d + 5)
        fleet, at, missing, gaps, (is_lo, is_hi, end_first, end_second, is_start) = _TrajectoryStaggeredSeparation._saved(ctx)
        g = torch.where(missing, torch.zeros_like(g_value), g_value)      # a NaN value: gradient 0
        need = ctx.needs_input_grad[2:]
        want_time = any(need[8 * c + 6] or need[8 * c + 7] for c in range(d)) or any(need[8 * d:])
        # (a bad vehicle's gap is NaN: not into its partners)
        g_gap = lambda c: torch.where(missing, torch.zeros_like(g), (2.0 * g) * gaps[c])      # noqa: E731
        bars, time_bar, shift_bar = [], None, None
        for bar, tau_bar in _fleet_vjp(fleet, at, need, want_time, g_gap):
            bars += bar
            if want_time:      # the pair's: its two vehicles', added in _TrajectorySeparation's order -- the same bits per pair and query
                share_first, share_second = at.per_pair(tau_bar)
                time_bar = share_first if time_bar is None else time_bar + share_first
                time_bar = time_bar + share_second
                shift_bar = share_second if shift_bar is None else shift_bar + share_second
        start_bar = lo_bar = hi_bar = None
        if want_time:
            zero = torch.zeros_like(time_bar)
            routed = lambda mask: torch.where(mask, time_bar, zero)      # noqa: E731
            _route_end_bars(bars, need, at, routed, end_first, end_second)
            lo_pair, hi_pair = routed(is_lo), routed(is_hi)
            if need[8 * d + 1]:
                lo_bar = lo_pair.sum(dim=1)
            if need[8 * d + 2]:
                hi_bar = hi_pair.sum(dim=1)
            if need[8 * d]:      # the second vehicle is at t' - delay, and the times that hold the delay move with it
                holds = is_start
                for mask in end_second:
                    holds = holds | mask
                delay_bar = routed(holds) - shift_bar
                start_bar = torch.where(at.signs > 0, at.through(-((delay_bar + lo_pair) + hi_pair)), at.through(delay_bar)).sum(dim=(2, 3))
        return (None, None) + tuple(bars) + (start_bar, lo_bar, hi_bar)

    @staticmethod
    def jvp(ctx, _t_d, _t_m, *tangents):
        d, m = ctx.d, ctx.m
        fleet, at, missing, gaps, (is_lo, is_hi, end_first, end_second, is_start) = _TrajectoryStaggeredSeparation._saved(ctx)
        first, second = at.slots[4], at.slots[5]
        dots = [_dense(t) for t in tangents[:8 * d]]
        zero = torch.zeros(missing.shape, dtype=torch.float64, device=at.tau.device)
        wide = lambda t: t.unsqueeze(1) if t is not None else zero      # noqa: E731
        start_dot = tangents[8 * d]
        first_dot = start_dot[:, first].unsqueeze(2) if start_dot is not None else zero
        delay_dot = (start_dot[:, second] - start_dot[:, first]).unsqueeze(2) + zero if start_dot is not None else zero
        time_dot = torch.where(is_lo, wide(tangents[8 * d + 1]) - first_dot, zero)
        time_dot = torch.where(is_hi, wide(tangents[8 * d + 2]) - first_dot, time_dot)
        for which, ends, shift in ((first, end_first, zero), (second, end_second, delay_dot)):
            for c in range(d):
                total = shift
                for t in (dots[8 * c + 6], dots[8 * c + 7]):
                    if t is not None:
                        total = total + t.reshape(-1, m)[:, which].unsqueeze(2)
                time_dot = torch.where(ends[c], total, time_dot)
        time_dot = torch.where(is_start, delay_dot, time_dot)
        tau_dot = torch.where(at.signs > 0, at.through(time_dot), at.through(time_dot - delay_dot)).reshape(at.tau.shape).contiguous()
        value_dot = zero
        for share in _fleet_jvp(fleet, at, gaps, dots, tau_dot):
            value_dot = value_dot + share
        return torch.where(missing, torch.full_like(zero, float("nan")), value_dot), None, None


def _check_fleet_start(n, m, start, who):
    """start: float64, (n, m) -- shape and type; the device comes after the windows' shapes (_check_fleet_start_device)."""
    _check_is_tensor("start", start, who)
    if start.dim() != 2 or tuple(start.shape) != (n, m):
        raise ValueError("%s: start must have shape (%d, %d) -- one start time per vehicle -- got %s" % (who, n, m, tuple(start.shape)))
    _check_is_float64("start", start, who)


def _check_fleet_start_device(start, device, who):
    if start.device != device:
        raise TypeError("%s: start is on %s; it must be on the fleet's device %s" % (who, start.device, device))


def _check_fleet_arguments(n, m, device, start, queries, who):
    """What comes after the fleet's own shapes and types: start's shape and type, queries() -- the checks of the windows (and the level),
    whose result is returned --, then start's device."""
    if start is not None:
        _check_fleet_start(n, m, start, who)
    checked = queries()
    if start is not None:
        _check_fleet_start_device(start, device, who)
    return checked


def _check_fleet_problem(pos, vel, synchronize, who, size=_check_fleet_size):
    """pos and vel of a fleet pipeline, shapes and types; returns (n, m, d).  size: the check of m."""
    if synchronize and vel is not None:
        raise ValueError(who + ": synchronize=True needs rest-to-rest vehicles; pass synchronize=False with end velocities")
    if not isinstance(pos, (list, tuple)) or len(pos) != 3:
        raise TypeError("%s: pos must be a list or tuple of three tensors (pos0, pos1, pos2)" % who)
    if vel is not None and (not isinstance(vel, (list, tuple)) or len(vel) != 2):
        raise TypeError("%s: vel must be None or a pair (vel0, vel2)" % who)
    for name, t in [("pos", t) for t in pos] + [("vel", v) for v in (vel or ()) if v is not None]:
        _check_is_tensor(name, t, who)
        if t.dim() != 3 or t.shape != pos[0].shape or not 1 <= t.shape[2] <= 3:
            raise ValueError("%s: every tensor must have one shape (n, m, d) with d in 1..3, got %s" % (who, tuple(t.shape)))
    n, m, d = pos[0].shape
    size(int(m), who)
    return n, int(m), d


def _solve_fleet(pos, vel, synchronize, gap_tol, max_iter, params):
    """One min_time_solve over the n m d axis problems of a fleet: (the fleet as trajectory_fleet_separation takes it, stretched where
    synchronize; the solution as (n, m, d), as the solve left it)"""
    n, m, d = pos[0].shape
    flat = lambda t: t.reshape(-1) if t is not None else None      # noqa: E731
    vel0, vel2 = (flat(v) for v in vel) if vel is not None else (None, None)
    solution = min_time_solve(*[flat(t) for t in pos], gap_tol=gap_tol, max_iter=max_iter, params=params, vel0=vel0, vel2=vel2)
    spline = list(pos) + [t.reshape(n, m, d) for t in solution[:3]]
    if synchronize:
        spline, _ = synchronize_axes([t.reshape(n * m, d) for t in spline])
        spline = [t.reshape(n, m, d) for t in spline]
    elif vel is not None:
        spline = spline + list(vel)
    return spline, tuple(t.reshape(n, m, d) for t in solution)


def _check_fleet(fleet, who, name="fleet", size=_check_fleet_size):
    """A fleet as trajectory_fleet_separation takes it: six or eight float64 tensors (n, m, d): shapes and types (the devices come after
    the windows' shapes: _check_fleet_devices).  Returns (n, m, d, the d splines as lists of eight (n m,) tensors in the table's order).
    name: what the messages call it; size: the check of m."""
    _check_spline_arg(name, fleet, who)
    pos0 = fleet[0]
    _check_is_tensor(name + ": pos0", pos0, who)
    if pos0.dim() != 3:
        raise ValueError("%s: %s: pos0 must have shape (n, m, d), got %s" % (who, name, tuple(pos0.shape)))
    n, m, d = pos0.shape
    if n == 0:
        raise ValueError(who + ": empty batch")
    size(int(m), who)
    if not 1 <= d <= 3:
        raise ValueError("%s: %s has %d axes; one, two or three are supported" % (who, name, d))
    names = ("pos0", "pos1", "pos2", "vel1", "duration0", "duration1", "vel0", "vel2")
    for field, t in zip(names, fleet):
        if t is None and field in ("vel0", "vel2"):
            continue
        _check_is_tensor(name + ": " + field, t, who)
        if t.shape != pos0.shape:
            raise ValueError("%s: %s: %s has shape %s, pos0 %s" % (who, name, field, tuple(t.shape), tuple(pos0.shape)))
        _check_is_float64(name + ": " + field, t, who)
    vel0, vel2 = fleet[6:] if len(fleet) == 8 else (None, None)
    table = list(fleet[:3]) + [vel0, vel2] + list(fleet[3:6])
    return n, int(m), d, [[t[:, :, c].reshape(n * m) if t is not None else None for t in table] for c in range(d)]


def _check_fleet_devices(fleet, who):
    for t in fleet:
        if t is not None and (t.device.type != "cuda" or t.device != fleet[0].device):
            raise TypeError("%s: fleet: a tensor is on %s; the fleet must be on one ROCm device" % (who, t.device))


def _check_fleet_windows(n, device, lo, hi, who):
    """lo, hi (None: -inf / +inf): float64, (n, k) -- one window per scene and query, for all its pairs -- or (k,); returned as (n, k)."""
    out, shapes = [], []
    for name, t in (("lo", lo), ("hi", hi)):
        if t is None:
            out.append(None)
            continue
        _check_is_tensor(name, t, who)
        _check_is_float64(name, t, who)
        if t.dim() == 1 and t.shape[0] > 0:
            t = t.unsqueeze(0).expand(n, t.shape[0])
        elif t.dim() != 2 or t.shape[0] != n or t.shape[1] == 0:
            raise ValueError("%s: %s must have shape (%d, k) or (k,) with k >= 1 -- a scene's window holds for all its pairs -- got %s"
                             % (who, name, n, tuple(t.shape)))
        if t.device != device:
            raise TypeError("%s: %s is on %s; it must be on the fleet's device %s" % (who, name, t.device, device))
        out.append(t)
        shapes.append((name, t.shape))
    if len(shapes) == 2 and shapes[0][1] != shapes[1][1]:
        raise ValueError("%s: lo has shape %s, hi %s" % (who, tuple(shapes[0][1]), tuple(shapes[1][1])))
    return out


def trajectory_fleet_separation(fleet, lo=None, hi=None, *, start=None):
    """trajectory_separation for every pair of a fleet, in one launch: n scenes of m vehicles (2..256) that move in d = 1, 2 or 3 axes, all
    vehicles of a scene on one clock.  fleet: a sequence of six tensors (pos0, pos1, pos2, vel1, duration0, duration1), or of eight with
    (vel0, vel2) appended, each (n, m, d) -- always three-dimensional -- float64 on one ROCm device.  lo, hi: (n, k), the windows of a
    scene for all its pairs, or (k,) for the same in every scene; None: -inf / +inf, both None: k = 1, the whole common domain of each
    pair.  Returns (sep_sq, t_closest), (n, pairs, k) each, pairs = m (m - 1) / 2 in fleet_pairs(m)'s order: [s, (i, j), q] is bit for bit
    what trajectory_separation gives for vehicles i and j of scene s, the window [lo, hi][s, q] and no delay -- its NaN rule (a vehicle
    with a bad duration makes exactly its m - 1 pairs NaN), domain, candidates and earliest-among-equals.

    One rp_trajectory_fleet_separation launch on the current stream; no pair-expanded tensor is made.  sep_sq is differentiable to first
    order in all fleet tensors, lo and hi, in both modes: per axis one rp_trajectory_eval launch and one rp_trajectory_eval_vjp (reverse)
    or rp_trajectory_eval_jvp (forward) launch on the n m splines at the returned times; every sum over pairs is a
    gather and a sum, so a gradient is the same bits in every run; a double backward raises torch's once_differentiable error.  At ties
    the derivative is that of the branch the forward pass found.  A NaN value has gradient 0 (forward mode: NaN).  The time is not
    differentiable.  Does not synchronise the host.

    start= (n, m), float64 on the fleet's device, gives every vehicle a start time of its own: vehicle v runs its
    spline over [start, start + T] of the scene's clock, on which lo, hi and t_closest then are.  [s, (i, j), q] is bit for bit
    trajectory_separation's value for vehicles i and j with delay = start_j - start_i over the window [lo - start_i, hi - start_i], and
    t_closest its time plus start_i; a NaN or infinite start makes exactly its vehicle's m - 1 pairs NaN, pairs never under way together
    are NaN.  One rp_trajectory_fleet_separation_staggered launch; sep_sq is differentiable in start as well, by the pair entry's rule
    for its delay, lo and hi.  start=None is the call without it: the same launches and the same bits."""
    who = "trajectory_fleet_separation"
    n, m, d, tables = _check_fleet(fleet, who)
    lo, hi = _check_fleet_arguments(n, m, fleet[0].device, start, lambda: _check_fleet_windows(n, fleet[0].device, lo, hi, who), who)
    _check_fleet_devices(fleet, who)
    if start is None:
        return _TrajectoryFleetSeparation.apply(d, m, *[t for table in tables for t in table], lo, hi)
    return _TrajectoryStaggeredSeparation.apply(d, m, *[t for table in tables for t in table], start, lo, hi)[:2]


def min_time_fleet_separation(pos, lo=None, hi=None, *, vel=None, synchronize=True, gap_tol=1e-8, max_iter=200, params=None, start=None):
    """min_time_solve of a fleet's axes, then trajectory_fleet_separation of the solutions.  pos: (pos0, pos1, pos2), (n, m, d) each: one
    solve over the n m d axis problems.  vel: (vel0, vel2), (n, m, d) each (None: rest to rest).  synchronize (the default): each
    vehicle's axes are stretched to its slowest first (synchronize_axes on (n m, d); rest to rest only: with end velocities given it
    raises ValueError).  lo, hi as trajectory_fleet_separation's.  Returns (sep_sq, t_closest, solution) with the solution
    min_time_solve's (vel1, duration0, duration1, iters, status) as (n, m, d), as the solve left them (before the stretch).  Plain
    composition: sep_sq is differentiable to first order in the positions, the end velocities, lo and hi, in both modes.  start= (n, m):
    trajectory_fleet_separation's start times, checked before the solve and differentiable like lo and hi."""
    who = "min_time_fleet_separation"
    n, m, d = _check_fleet_problem(pos, vel, synchronize, who)
    # before the solve: a bad query costs none
    lo, hi = _check_fleet_arguments(n, m, pos[0].device, start, lambda: _check_fleet_windows(n, pos[0].device, lo, hi, who), who)
    spline, solution = _solve_fleet(pos, vel, synchronize, gap_tol, max_iter, params)
    return tuple(trajectory_fleet_separation(spline, lo, hi, start=start)) + (solution,)


# ---- when two vehicles moving in several axes first come within a distance ----
class _TrajectoryContact(torch.autograd.Function):
    """(time, rate) of the first time in the window at which f(t) = sum over the axes of (pos_Ac(t) - pos_Bc(t - delay))^2 is at the level:
    the time is differentiable to first order in all 16 d spline inputs, the level and the delay through the evaluator's derivative launches
    on each axis' two splines -- f(theta, time) = level gives
    d time = (d level - sum of 2 D_c (d pos_Ac - d pos_Bc + vel_Bc d delay)) / rate with rate = f'(time).  Inputs: d, then A's 8 d tensors
    (axis-major), B's 8 d, then level_sq, lo, hi, delay.  lo and hi only choose the branch.  rate is for the backward and is not
    differentiable."""

    @staticmethod
    def forward(d, *inputs):
        a, b = [_dense(t) for t in inputs[:8 * d]], [_dense(t) for t in inputs[8 * d:16 * d]]
        level, lo, hi, delay = (_dense(t) for t in inputs[16 * d:])
        (n, k), device = level.shape, inputs[0].device
        time, rate = _empty((n, k), device), _empty((n, k), device)
        _enqueue(capi.trajectory_contact, device, n, k, d, a, b, level, lo, hi, delay, time, rate)
        return time, rate

    @staticmethod
    def setup_context(ctx, inputs, output):
        d = ctx.d = inputs[0]
        rest = inputs[1:]      # neither derivative reads the level, lo or hi
        _keep(ctx, rest, output, dead=output[1:], given=[t is not None for t in rest[:16 * d]] + [False, False, False, rest[16 * d + 3] is not None])

    @staticmethod
    def _saved(ctx):
        """(A's and B's d lists of eight tensors; A's times, 0 where there is no contact, and B's, those minus the delay; rate; where there
        is no contact; the d gaps D_c at those times)"""
        d = ctx.d
        inputs, (time, rate) = _kept(ctx)
        a, b = _axis_tables(inputs, d)
        delay = inputs[16 * d + 3]
        missing = torch.isnan(time)
        zero = torch.zeros_like(time)
        t_a = torch.where(missing, zero, time).contiguous()
        t_b = torch.where(missing, zero, time - delay if delay is not None else time).contiguous()
        return a, b, t_a, t_b, rate, missing, _pair_gaps(a, b, t_a, t_b)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_time, _g_rate):
        d = ctx.d
        if g_time is None:
            return (None,) * (16 * d + 5)
        a, b, t_a, t_b, rate, missing, gaps = _TrajectoryContact._saved(ctx)
        need = ctx.needs_input_grad[1:]
        w = torch.where(missing, torch.zeros_like(t_a), g_time / rate)      # an unreached level: gradient 0
        n, k = t_a.shape
        bars, delay_bar = [None] * (16 * d), None
        for c in range(d):
            g_pos = ((2.0 * w) * gaps[c]).contiguous()
            bar = _bars(need[8 * c:8 * c + 8], n, t_a.device)
            if any(x is not None for x in bar):
                _enqueue(capi.trajectory_eval_vjp, t_a.device, n, k, a[c], t_a, -g_pos, None, None, bar, None)
            bars[8 * c:8 * c + 8] = bar
            first = 8 * (d + c)
            bar = _bars(need[first:first + 8], n, t_a.device)
            tau_bar = _empty(t_a.shape, t_a.device) if need[16 * d + 3] else None
            if tau_bar is not None or any(x is not None for x in bar):      # B is at time - delay
                _enqueue(capi.trajectory_eval_vjp, t_a.device, n, k, b[c], t_b, g_pos, None, None, bar, tau_bar)
            bars[first:first + 8] = bar
            if tau_bar is not None:
                delay_bar = -tau_bar if delay_bar is None else delay_bar - tau_bar
        return (None,) + tuple(bars) + (w if need[16 * d] else None, None, None, delay_bar)

    @staticmethod
    def jvp(ctx, _t_d, *tangents):
        d = ctx.d
        a, b, t_a, t_b, rate, missing, gaps = _TrajectoryContact._saved(ctx)
        dots = [_dense(t) for t in tangents[:16 * d]]
        level_dot, delay_dot = tangents[16 * d], tangents[16 * d + 3]
        tau_dot_b = (-delay_dot).contiguous() if delay_dot is not None else None
        total = level_dot if level_dot is not None else torch.zeros_like(t_a)
        for c in range(d):
            pos_a, pos_b = _empty(t_a.shape, t_a.device), _empty(t_a.shape, t_a.device)
            _enqueue(capi.trajectory_eval_jvp, t_a.device, *t_a.shape, a[c], t_a, dots[8 * c:8 * c + 8], None, pos_a, None, None)
            _enqueue(capi.trajectory_eval_jvp, t_a.device, *t_a.shape, b[c], t_b, dots[8 * (d + c):8 * (d + c) + 8], tau_dot_b, pos_b, None, None)
            total = total - (2.0 * gaps[c]) * (pos_a - pos_b)
        return torch.where(missing, torch.full_like(t_a, float("nan")), total / rate), None


def trajectory_contact(a, b, radius=None, lo=None, hi=None, delay=None, *, level_sq=None):
    """The first time at which two vehicles that move in d = 1, 2 or 3 axes come within `radius` of each other: the earliest t in the
    windows of time [lo, hi] at which f(t) = sum over the axes of (pos_a,c(t) - pos_b,c(t - delay))^2 is at radius^2 -- the inverse of
    trajectory_separation's f as trajectory_meeting is of trajectory_gap's D.  a, b, lo, hi, delay: exactly trajectory_separation's.
    radius: (n, k), or (k,) for the same radii in every problem; the level is radius * radius, formed in torch, so the radius gets its
    gradient by the chain rule.  level_sq= may be given instead of radius (giving both, or neither, is a TypeError): the level itself, in
    units of squared distance; a negative one is legal and never reached.  Returns t_contact (on a's clock), (n, k): NaN where f does not
    reach the level in the window clamped to the 2 d splines' common domain (no extrapolation), where the clamped window is empty, where the
    level is NaN or infinite or the delay NaN or infinite, and for a problem any of whose 2 d splines has a duration that is not finite or
    not > 0.

    One rp_trajectory_contact launch on the current stream (include/rp_batch.h: each piece between knots is cut at the stationary points of
    f, the first of the monotone sub-pieces whose end values hold the level is solved by a bracketed Newton search with a fixed trip
    bound; a level within rounding of an extreme of f may give the touch, a later contact, or NaN).  Differentiable to first order in all
    16 d spline inputs, the level and the delay, d time = (d level - sum of 2 D_c (d pos_a,c - d pos_b,c + vel_b,c d delay)) / rate with
    rate = f'(time): per axis one rp_trajectory_eval launch on each spline, and one rp_trajectory_eval_vjp (reverse mode) or
    rp_trajectory_eval_jvp (forward mode) launch on each; a double backward raises torch's once_differentiable
    error.  lo and hi get no gradient: the time depends on them through the branch only.  An unreached level has gradient 0 (forward
    mode: NaN, as the time); where rate is 0 (a touch) there is no derivative and the result is inf or NaN; the time jumps where an
    earlier extreme of f passes through the level.  Does not synchronise the host."""
    who = "trajectory_contact"
    if (radius is None) == (level_sq is None):
        raise TypeError(who + ": give either radius or level_sq=, not %s" % ("both" if radius is not None else "neither"))
    _check_spline_arg("a", a, who)
    _check_spline_arg("b", b, who)
    d, axes_a = _check_axes("a", a, who)
    d_b, axes_b = _check_axes("b", b, who)
    if d_b != d:
        raise ValueError("%s: a has %d axes, b %d" % (who, d, d_b))
    tables_a = [_spline_table("a, axis %d" % c, s, who) for c, s in enumerate(axes_a)]
    tables_b = [_spline_table("b, axis %d" % c, s, who) for c, s in enumerate(axes_b)]
    _check_same_batch(tables_a[0][0], tables_b[0][0], who)
    level = _check_contact_level(tables_a[0][0], radius, level_sq, who)
    level, lo, hi, delay = _check_named_queries(tables_a[0][0], (("radius" if radius is not None else "level_sq", level), ("lo", lo), ("hi", hi),
                                                                 ("delay", delay)), who)
    flat = [t for table in tables_a + tables_b for t in table]
    return _TrajectoryContact.apply(d, *flat, level, lo, hi, delay)[0]


def _check_contact_level(pos0, radius, level_sq, who):
    """The level of trajectory_contact: radius * radius, or level_sq (exactly one is given)."""
    if radius is None:
        return level_sq
    _check_tau(pos0, radius, who, "radius")
    return radius * radius


def min_time_contact(pos_a, pos_b, radius=None, lo=None, hi=None, delay=None, *, level_sq=None, vel_a=None, vel_b=None, synchronize=True,
                     gap_tol=1e-8, max_iter=200, params=None):
    """min_time_solve of two vehicles' axes, then trajectory_contact of the two solutions: min_time_separation's composition -- pos_a,
    pos_b, vel_a, vel_b, synchronize and the solutions returned are its -- with trajectory_contact's radius (or level_sq=), lo, hi and delay.
    Returns (t_contact, solution_a, solution_b).  Plain composition: the times are differentiable to first order in both vehicles' positions
    and end velocities, in the radius and the delay, in both modes."""
    who = "min_time_contact"
    if (radius is None) == (level_sq is None):
        raise TypeError(who + ": give either radius or level_sq=, not %s" % ("both" if radius is not None else "neither"))
    flat = _check_axis_vehicles(pos_a, pos_b, vel_a, vel_b, synchronize, who)
    pos0 = pos_a[0][:, 0]      # before the solves: a bad query costs none
    level = _check_contact_level(pos0, radius, level_sq, who)
    level, lo, hi, delay = _check_named_queries(pos0, (("radius" if radius is not None else "level_sq", level), ("lo", lo), ("hi", hi),
                                                       ("delay", delay)), who)
    splines, solutions = _solve_axis_vehicles(pos_a, pos_b, flat, synchronize, gap_tol, max_iter, params)
    return trajectory_contact(splines[0], splines[1], None, lo, hi, delay, level_sq=level), solutions[0], solutions[1]


# ---- the first contact of every pair of a fleet ----
def _fleet_level(level):
    """(the level as the entry reads it, whether it is one per pair): (n, k) or (n, pairs, k)"""
    per_pair = level.dim() == 3
    if per_pair and _plain(level).data_ptr() % 16:      # a view that starts in the middle of a 16-byte vector
        level = level.clone()
    return level, per_pair


def _level_bar(ctx, w):
    return w if ctx.per_pair else w.sum(dim=1)


def _level_dot(ctx, level_dot, rate):
    if level_dot is None:
        return torch.zeros_like(rate)
    return level_dot if ctx.per_pair else level_dot.unsqueeze(1)


class _TrajectoryFleetContact(torch.autograd.Function):
    """(time, rate), (n, pairs, k) each, of the first time in the scene's window at which a pair's squared distance is at the level.  Inputs:
    d, m, the fleet's 8 d tensors, level_sq -- (n, k): one level for all pairs of a scene, or (n, pairs, k): one per pair --, lo, hi
    (n, k).  The time is differentiable to first order in all 8 d fleet inputs and the level by _TrajectoryContact's implicit-function
    formula, d time = (d level - sum of 2 D_c (d pos_first,c - d pos_second,c)) / rate, routed per vehicle.  lo and
    hi only choose the branch.  rate is for the backward and is not differentiable."""

    @staticmethod
    def forward(d, m, *inputs):
        level, lo, hi = (_dense(t) for t in inputs[8 * d:])
        level, per_pair = _fleet_level(level)
        return _fleet_forward(capi.trajectory_fleet_contact, d, m, inputs, level.shape[0], level.shape[-1], 2, level, int(per_pair), lo, hi)

    @staticmethod
    def setup_context(ctx, inputs, output):
        d = inputs[0]
        ctx.per_pair = inputs[2 + 8 * d].dim() == 3
        _fleet_setup(ctx, inputs, 8 * d, output[1:], output)      # neither derivative reads the level, lo or hi

    @staticmethod
    def _saved(ctx):
        """(the d lists of eight tensors; _fleet_times; rate; where there is no contact, (n, pairs, k); the d gaps D_c)"""
        fleet, _, (time, rate) = _fleet_kept(ctx)
        missing = torch.isnan(time)
        at = _fleet_times(ctx.m, time, missing)
        return fleet, at, rate, missing, _fleet_gaps(fleet, at)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_time, _g_rate):
        d = ctx.d
        if g_time is None:
            return (None,) * (8 * d + 5)
        fleet, at, rate, missing, gaps = _TrajectoryFleetContact._saved(ctx)
        need = ctx.needs_input_grad[2:]
        zero = torch.zeros_like(rate)
        w = torch.where(missing, zero, g_time / rate)      # an unreached level: gradient 0
        # (a bad vehicle's gap is NaN: not into its partners)
        g_gap = lambda c: torch.where(missing, zero, -((2.0 * w) * gaps[c]))      # noqa: E731
        bars = [x for bar, _ in _fleet_vjp(fleet, at, need, False, g_gap) for x in bar]
        level_bar = _level_bar(ctx, w) if need[8 * d] else None
        return (None, None) + tuple(bars) + (level_bar, None, None)

    @staticmethod
    def jvp(ctx, _t_d, _t_m, *tangents):
        d = ctx.d
        fleet, at, rate, missing, gaps = _TrajectoryFleetContact._saved(ctx)
        dots = [_dense(t) for t in tangents[:8 * d]]
        total = _level_dot(ctx, tangents[8 * d], rate)
        for share in _fleet_jvp(fleet, at, gaps, dots, None):
            total = total - share
        return torch.where(missing, torch.full_like(rate, float("nan")), total / rate), None


def _cull_workspace(n, m, k, d, device, staggered):
    """The culled entries' workspace (staggered: of those with start times) as a torch allocation on the current stream: (tensor, bytes)"""
    ask = capi.trajectory_fleet_contact_staggered_culled_workspace if staggered else capi.trajectory_fleet_contact_culled_workspace
    size = ask(n, m, k, d)
    return torch.empty(size, dtype=torch.uint8, device=device), size


def _culled_forward(entry, d, m, inputs):
    """The forward of the two functions with the broad phase in front: behind the fleet's tensors the inputs are (level_sq, lo, hi), or
    (start, level_sq, lo, hi) and one output more; the workspace's address and size follow the entry's other arguments."""
    *start, level, lo, hi = (_dense(t) for t in inputs[8 * d:])
    level, per_pair = _fleet_level(level)
    n, k = level.shape[0], level.shape[-1]
    work, size = _cull_workspace(n, m, k, d, inputs[0].device, bool(start))
    return _fleet_forward(entry, d, m, inputs, n, k, 2 + len(start), *start, level, int(per_pair), lo, hi, tail=(work, size))


class _TrajectoryFleetContactCulled(_TrajectoryFleetContact):
    """_TrajectoryFleetContact with the broad phase in front of the forward: rp_trajectory_fleet_contact_culled gives
    the same bits in time and rate, so what is saved and both derivative rules are the parent's, unchanged."""

    @staticmethod
    def forward(d, m, *inputs):
        return _culled_forward(capi.trajectory_fleet_contact_culled, d, m, inputs)


class _TrajectoryStaggeredContact(torch.autograd.Function):
    """_TrajectoryFleetContact with a start time per vehicle: (the time on the scene's clock, the time on the clock of the pair's first
    vehicle, rate), (n, pairs, k) each.  Inputs: d, m, the fleet's 8 d tensors, start (n, m), level_sq, lo, hi.  Pair (i, j) is
    _TrajectoryContact's query with delay = start_j - start_i over [lo - start_i, hi - start_i]; the scene-clock time is its time t' plus
    start_i and is differentiable by its implicit-function formula routed per vehicle: vehicle i is evaluated at t', vehicle j at
    t' - delay, delay_bar is minus the second vehicle's tau_bar, start_j gets delay_bar and start_i minus delay_bar plus the time's own
    +1.  lo and hi only choose the branch; the local time and the rate are not differentiable."""

    @staticmethod
    def forward(d, m, *inputs):
        start, level, lo, hi = (_dense(t) for t in inputs[8 * d:])
        level, per_pair = _fleet_level(level)
        return _fleet_forward(capi.trajectory_fleet_contact_staggered, d, m, inputs, level.shape[0], level.shape[-1], 3, start, level,
                              int(per_pair), lo, hi)

    @staticmethod
    def setup_context(ctx, inputs, output):
        d = inputs[0]
        ctx.per_pair = inputs[3 + 8 * d].dim() == 3
        _fleet_setup(ctx, inputs, 8 * d, output[1:], (inputs[2 + 8 * d], output[1], output[2]))      # as _TrajectoryFleetContact, and the start

    @staticmethod
    def _saved(ctx):
        fleet, _, (start, local, rate) = _fleet_kept(ctx)
        missing = torch.isnan(local)
        at = _fleet_times(ctx.m, local, missing, start)
        return fleet, at, rate, missing, _fleet_gaps(fleet, at)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_time, _g_local, _g_rate):
        d = ctx.d
        if g_time is None:
            return (None,) * (8 * d + 6)
        fleet, at, rate, missing, gaps = _TrajectoryStaggeredContact._saved(ctx)
        need = ctx.needs_input_grad[2:]
        zero = torch.zeros_like(rate)
        own = torch.where(missing, zero, g_time)      # time = t' + start_i
        w = torch.where(missing, zero, g_time / rate)      # an unreached level: gradient 0
        # (a bad vehicle's gap is NaN: not into its partners)
        g_gap = lambda c: torch.where(missing, zero, -((2.0 * w) * gaps[c]))      # noqa: E731
        bars, delay_bar = [], None
        for bar, tau_bar in _fleet_vjp(fleet, at, need, need[8 * d], g_gap):
            bars += bar
            if tau_bar is not None:      # the second vehicle is at t' - delay
                share = at.per_pair(tau_bar)[1]
                delay_bar = -share if delay_bar is None else delay_bar - share
        start_bar = level_bar = None
        if need[8 * d]:
            start_bar = torch.where(at.signs > 0, at.through(own - delay_bar), at.through(delay_bar)).sum(dim=(2, 3))
        if need[8 * d + 1]:
            level_bar = _level_bar(ctx, w)
        return (None, None) + tuple(bars) + (start_bar, level_bar, None, None)

    @staticmethod
    def jvp(ctx, _t_d, _t_m, *tangents):
        d = ctx.d
        fleet, at, rate, missing, gaps = _TrajectoryStaggeredContact._saved(ctx)
        first, second = at.slots[4], at.slots[5]
        dots = [_dense(t) for t in tangents[:8 * d]]
        start_dot = tangents[8 * d]
        total = _level_dot(ctx, tangents[8 * d + 1], rate)
        tau_dot = None
        if start_dot is not None:      # the second vehicle's time moves against the delay
            zero = torch.zeros_like(rate)
            delay_dot = (start_dot[:, second] - start_dot[:, first]).unsqueeze(2) + zero
            tau_dot = torch.where(at.signs > 0, at.through(zero), at.through(-delay_dot)).reshape(at.tau.shape).contiguous()
        for share in _fleet_jvp(fleet, at, gaps, dots, tau_dot):
            total = total - share
        time_dot = total / rate
        if start_dot is not None:
            time_dot = time_dot + start_dot[:, first].unsqueeze(2)
        return torch.where(missing, torch.full_like(rate, float("nan")), time_dot), None, None


class _TrajectoryStaggeredContactCulled(_TrajectoryStaggeredContact):
    """_TrajectoryStaggeredContact with the broad phase in front of the forward:
    rp_trajectory_fleet_contact_staggered_culled gives the same bits in the three outputs, so what is saved and both derivative rules are
    the parent's, unchanged."""

    @staticmethod
    def forward(d, m, *inputs):
        return _culled_forward(capi.trajectory_fleet_contact_staggered_culled, d, m, inputs)


def _check_broad_phase(broad_phase, start, who):
    """broad_phase: False, True (not with start=) or "staggered" (only with start=)."""
    if isinstance(broad_phase, str):
        if broad_phase != "staggered":
            raise ValueError('%s: broad_phase must be False, True or "staggered", got %r' % (who, broad_phase))
        if start is None:
            raise ValueError('%s: broad_phase="staggered" needs start=; without start times broad_phase=True is the broad phase' % who)
    elif broad_phase and start is not None:
        raise ValueError(who + ': broad_phase=True does not take start=; broad_phase="staggered" is the broad phase of the staggered entries')


def _check_fleet_level(n, pairs, radius, level_sq, who):
    """The level of trajectory_fleet_contact, shape and type (the device comes after the windows' shapes): radius or level_sq, float64,
    (n, k), (k,) -- one level for all pairs of a scene -- or (n, pairs, k) -- one per pair.  Returns (its name, the level in units of
    squared distance as (n, k) or (n, pairs, k))."""
    name, t = ("radius", radius) if radius is not None else ("level_sq", level_sq)
    _check_is_tensor(name, t, who)
    _check_is_float64(name, t, who)
    if t.dim() == 1 and t.shape[0] > 0:
        t = t.unsqueeze(0).expand(n, t.shape[0])
    elif not ((t.dim() == 2 and t.shape[0] == n and t.shape[1] > 0) or (t.dim() == 3 and t.shape[:2] == (n, pairs) and t.shape[2] > 0)):
        raise ValueError("%s: %s must have shape (%d, k) or (k,) -- a scene's level for all its pairs -- or (%d, %d, k) -- one per pair -- "
                         "with k >= 1, got %s" % (who, name, n, n, pairs, tuple(t.shape)))
    return name, (t * t if radius is not None else t)


def _check_fleet_queries(n, m, device, radius, level_sq, lo, hi, who):
    """The level and the windows of a fleet's contact query: shapes and types before devices.  Returns (level, lo, hi)."""
    name, level = _check_fleet_level(n, m * (m - 1) // 2, radius, level_sq, who)
    lo, hi = _check_fleet_windows(n, device, lo, hi, who)
    for other, t in (("lo", lo), ("hi", hi)):
        if t is not None and t.shape[1] != level.shape[-1]:
            raise ValueError("%s: %s has %d queries per scene, %s %d" % (who, name, level.shape[-1], other, t.shape[1]))
    if level.device != device:
        raise TypeError("%s: %s is on %s; it must be on the fleet's device %s" % (who, name, level.device, device))
    return level, lo, hi


def trajectory_fleet_contact(fleet, radius=None, lo=None, hi=None, *, level_sq=None, start=None, broad_phase=False):
    """trajectory_contact for every pair of a fleet, in one launch: the first time in a scene's windows [lo, hi] at which two of its
    vehicles come within `radius` of each other.  fleet, lo, hi: exactly trajectory_fleet_separation's.  radius: (n, k), or (k,) for the
    same in every scene -- one radius for all pairs of a scene --, or (n, pairs, k) -- one per pair, what vehicles of different sizes need:
    r_i + r_j, formed by the caller.  The level is radius * radius, formed in torch, so the radius gets its gradient by the chain rule.
    level_sq= may be given instead of radius (giving both, or neither, is a TypeError): the level itself, in units of squared distance, in
    the same shapes.  Returns t_contact, (n, pairs, k), pairs = m (m - 1) / 2 in fleet_pairs(m)'s order: [s, (i, j), q] is bit for bit what
    trajectory_contact gives for vehicles i and j of scene s, the window [lo, hi][s, q], that query's level and no delay -- NaN where the
    pair does not reach the level in the window, and its NaN rule (a vehicle with a bad duration makes exactly its m - 1 pairs NaN).

    One rp_trajectory_fleet_contact launch on the current stream; no pair-expanded tensor is made.  Differentiable to first order in all
    fleet tensors and the level, in both modes, d time = (d level - sum of 2 D_c (d pos_i,c - d pos_j,c)) / rate: per axis one
    rp_trajectory_eval launch and one rp_trajectory_eval_vjp (reverse) or rp_trajectory_eval_jvp (forward) launch on the n m splines at
    the returned times; every sum over pairs is a gather and a sum, so a gradient is the same bits in every run; a
    double backward raises torch's once_differentiable error.  lo and hi get no gradient.  An unreached level has gradient 0 (forward
    mode: NaN, as the time); where rate is 0 (a touch) the result is inf or NaN.  fleet_first_contact gives the scene's first contact and
    its pair.  Does not synchronise the host.

    start= (n, m), float64 on the fleet's device: trajectory_fleet_separation's start times.  lo, hi and t_contact
    are then on the scene's clock: [s, (i, j), q] is trajectory_contact's time, bit for bit, for vehicles i and j with delay = start_j -
    start_i over the window [lo - start_i, hi - start_i], plus start_i.  One rp_trajectory_fleet_contact_staggered launch; the time is
    differentiable in start as well.  start=None is the call without it: the same launches and the same bits.

    broad_phase=True puts a bounding-box cull in front of the search: one rp_trajectory_fleet_contact_culled call
    -- per vehicle, axis and query the position's box over the window, per pair a lower bound of the boxes' distance with a proved margin,
    NaN written directly for the pairs whose bound is above the level in all k queries, and the search over a device-side list of the
    rest.  The same bits out, NaN included, hence the same gradients; the time goes with the number of near pairs and not with m^2.  The
    workspace is a torch allocation on the current stream.  Not with start= (ValueError).  False is the call without it: the same
    launches and the same bits as before.

    broad_phase="staggered" is the broad phase with start= (without start= a ValueError): one
    rp_trajectory_fleet_contact_staggered_culled call.  A query is out when the two vehicles are never under way together in its window
    -- decided exactly, by the search's own operations -- or when their boxes, each over the window on its own clock, are far; a pair all
    of whose queries are out gets its NaN without a search.  The same bits out, hence the same gradients, start's included."""
    who = "trajectory_fleet_contact"
    if (radius is None) == (level_sq is None):
        raise TypeError(who + ": give either radius or level_sq=, not %s" % ("both" if radius is not None else "neither"))
    _check_broad_phase(broad_phase, start, who)
    n, m, d, tables = _check_fleet(fleet, who)
    level, lo, hi = _check_fleet_arguments(n, m, fleet[0].device, start,
                                           lambda: _check_fleet_queries(n, m, fleet[0].device, radius, level_sq, lo, hi, who), who)
    _check_fleet_devices(fleet, who)
    if start is None:
        function = _TrajectoryFleetContactCulled if broad_phase else _TrajectoryFleetContact
        return function.apply(d, m, *[t for table in tables for t in table], level, lo, hi)[0]
    function = _TrajectoryStaggeredContactCulled if broad_phase else _TrajectoryStaggeredContact      # (with start=: "staggered" or False)
    return function.apply(d, m, *[t for table in tables for t in table], start, level, lo, hi)[0]


def min_time_fleet_contact(pos, radius=None, lo=None, hi=None, *, level_sq=None, vel=None, synchronize=True, gap_tol=1e-8, max_iter=200,
                           params=None, start=None, broad_phase=False):
    """min_time_solve of a fleet's axes, then trajectory_fleet_contact of the solutions: min_time_fleet_separation's composition -- pos,
    vel, synchronize and the solution returned are its -- with trajectory_fleet_contact's radius (or level_sq=), lo and hi.  Returns
    (t_contact, solution).  Plain composition: the times are differentiable to first order in the positions, the end velocities and the
    radius, in both modes.  start= (n, m): trajectory_fleet_contact's start times, checked before the solve and differentiable.
    broad_phase=True: trajectory_fleet_contact's bounding-box cull in front of the search; the same bits; not with start=.
    broad_phase="staggered": its broad phase with start=; the same bits."""
    who = "min_time_fleet_contact"
    if (radius is None) == (level_sq is None):
        raise TypeError(who + ": give either radius or level_sq=, not %s" % ("both" if radius is not None else "neither"))
    _check_broad_phase(broad_phase, start, who)
    n, m, d = _check_fleet_problem(pos, vel, synchronize, who)
    # before the solve: a bad query costs none
    level, lo, hi = _check_fleet_arguments(n, m, pos[0].device, start,
                                           lambda: _check_fleet_queries(n, m, pos[0].device, radius, level_sq, lo, hi, who), who)
    spline, solution = _solve_fleet(pos, vel, synchronize, gap_tol, max_iter, params)
    return trajectory_fleet_contact(spline, None, lo, hi, level_sq=level, start=start, broad_phase=broad_phase), solution


def _with_start(entry, staggered_entry, start):
    """(the entry to call, what to put behind its fleet table): the plain one and nothing, or with start= the staggered one and the start's address"""
    return (entry, ()) if start is None else (staggered_entry, (_dense(start.detach()).data_ptr(),))


def fleet_contact_candidates(fleet, radius=None, lo=None, hi=None, *, level_sq=None, start=None):
    """The broad phase of trajectory_fleet_contact(..., broad_phase=True) alone: a (n, pairs) bool tensor, in fleet_pairs(m)'s order, True
    where the pair would go to the search and False where its position boxes over the window prove, with the margin of DESIGN.md section
    30, that it is further apart than the level in all k queries -- trajectory_fleet_contact's times of such a pair are NaN.  A kept pair
    need not have a contact.  fleet, radius (or level_sq=), lo and hi: exactly trajectory_fleet_contact's.  One
    rp_trajectory_fleet_contact_candidates call on the current stream: boxes, sieve, no search.  Not differentiable.  start= (n, m):
    trajectory_fleet_contact's start times; the flags are then those of broad_phase="staggered" (DESIGN.md section 31), one
    rp_trajectory_fleet_contact_staggered_candidates call.  start=None: exactly the call without it."""
    who = "fleet_contact_candidates"
    if (radius is None) == (level_sq is None):
        raise TypeError(who + ": give either radius or level_sq=, not %s" % ("both" if radius is not None else "neither"))
    n, m, d, tables = _check_fleet(fleet, who)
    device = fleet[0].device
    level, lo, hi = _check_fleet_arguments(n, m, device, start, lambda: _check_fleet_queries(n, m, device, radius, level_sq, lo, hi, who), who)
    _check_fleet_devices(fleet, who)
    with torch.no_grad():
        level, per_pair = _fleet_level(_dense(level.detach()))
        lo, hi = (_dense(t.detach()) if t is not None else None for t in (lo, hi))
        k = level.shape[-1]
        splines = [_dense(t.detach()) if t is not None else None for table in tables for t in table]
        kept = torch.empty((n, m * (m - 1) // 2), dtype=torch.uint8, device=device)
        work, size = _cull_workspace(n, m, k, d, device, start is not None)
        entry, with_start = _with_start(capi.trajectory_fleet_contact_candidates, capi.trajectory_fleet_contact_staggered_candidates, start)
        _enqueue(entry, device, n, m, k, d, splines, *with_start, level, int(per_pair), lo, hi, work, size, kept)
    return kept != 0


def trajectory_fleet_reach(fleet, lo=None, hi=None, *, start=None):
    """How far every vehicle of a fleet gets in every axis: (box_min, box_max), (n, m, k, d) each -- the least and greatest position of
    vehicle v of scene s in axis c over the scene's window [lo, hi][s, q], bit for bit trajectory_extrema's pos_min and pos_max of that
    spline and window (its clamp to [0, T]; NaN for an empty clamped window and for a vehicle with a bad duration).  fleet, lo, hi:
    exactly trajectory_fleet_separation's; both windows None: k = 1, each spline's whole time.  One rp_trajectory_fleet_reach launch on
    the current stream; no window tensor repeated per vehicle is made.  These are the boxes of trajectory_fleet_contact's broad phase
    (DESIGN.md section 30).  Not differentiable: trajectory_extrema is the differentiable form.  start= (n, m): trajectory_fleet_contact's
    start times; vehicle v's window is then [lo - start_v, hi - start_v], on its own clock, one
    rp_trajectory_fleet_reach_staggered launch.  start=None: exactly the call without it."""
    who = "trajectory_fleet_reach"
    n, m, d, tables = _check_fleet(fleet, who)
    device = fleet[0].device
    lo, hi = _check_fleet_arguments(n, m, device, start, lambda: _check_fleet_windows(n, device, lo, hi, who), who)
    _check_fleet_devices(fleet, who)
    with torch.no_grad():
        lo, hi = (_dense(t.detach()) if t is not None else None for t in (lo, hi))
        k = next((t.shape[1] for t in (lo, hi) if t is not None), 1)
        splines = [_dense(t.detach()) if t is not None else None for table in tables for t in table]
        size = n * m * k
        flat = torch.empty((2, d, size + (size & 1)), dtype=torch.float64, device=device)      # every array starts on a 16-byte boundary
        box = flat[:, :, :size].unflatten(2, (n, m, k))      # a view: axis c's (n, m, k) array is contiguous
        entry, with_start = _with_start(capi.trajectory_fleet_reach, capi.trajectory_fleet_reach_staggered, start)
        _enqueue(entry, device, n, m, k, d, splines, *with_start, lo, hi, [box[0, c] for c in range(d)], [box[1, c] for c in range(d)])
    return box[0].permute(1, 2, 3, 0), box[1].permute(1, 2, 3, 0)


def fleet_first_contact(t_contact):
    """The first contact of each scene: (t_first, pair), (n, k) each, of trajectory_fleet_contact's (n, pairs, k) times.  t_first is the
    earliest finite time over the scene's pairs, NaN if no pair has one; pair is the int64 index into fleet_pairs(m) of the pair that
    attains it -- the lowest at ties --, -1 where there is none.  Plain torch on any device: the winner is selected by a one-hot mask and
    a sum over the pairs, so t_first is differentiable, its gradient goes to exactly the winning (pair, query) entry, and nothing adds
    with atomics: the same bits in every run."""
    who = "fleet_first_contact"
    _check_is_tensor("t_contact", t_contact, who)
    if t_contact.dim() != 3 or t_contact.shape[1] == 0 or not t_contact.is_floating_point():
        raise ValueError("%s: t_contact must be a floating-point tensor of shape (n, pairs, k), got %s %s"
                         % (who, t_contact.dtype, tuple(t_contact.shape)))
    pairs = t_contact.shape[1]
    index = torch.arange(pairs, device=t_contact.device).reshape(1, pairs, 1)
    finite = torch.isfinite(t_contact.detach())
    least = torch.where(finite, t_contact.detach(), torch.full_like(t_contact, float("inf"))).amin(dim=1, keepdim=True)
    pair = torch.where(finite & (t_contact.detach() == least), index, torch.full_like(index, pairs)).amin(dim=1)      # the lowest at ties
    any_finite = finite.any(dim=1)
    pair = torch.where(any_finite, pair, torch.full_like(pair, -1))
    one_hot = index == pair.unsqueeze(1)
    t_first = torch.where(one_hot, t_contact, torch.zeros_like(t_contact)).sum(dim=1)
    return torch.where(any_finite, t_first, torch.full_like(t_first, float("nan"))), pair


# ---- the vehicles of one fleet against the vehicles of another ----
def _check_cross_size(m, who):
    if isinstance(m, bool) or not isinstance(m, int):
        raise TypeError("%s: m_a and m_b must be ints, got %s" % (who, type(m).__name__))
    if not 1 <= m <= CROSS_MOST:
        raise ValueError("%s: a fleet holds 1..%d vehicles per scene, got %d" % (who, CROSS_MOST, m))


def cross_pairs(m_a, m_b, device=None):
    """The pairs (i, j) of m_a vehicles of fleet A against m_b of fleet B (1..32768 each) in the order of trajectory_cross_separation's
    outputs -- row-major, pair r = (r // m_b, r % m_b): a (2, m_a m_b) int64 tensor on `device`, row 0 the vehicle of A, row 1 that of B."""
    _check_cross_size(m_a, "cross_pairs")
    _check_cross_size(m_b, "cross_pairs")
    r = torch.arange(m_a * m_b, dtype=torch.int64, device=device)
    return torch.stack((r // m_b, r % m_b))


def static_fleet(points, duration=1.0):
    """The spline tensors of vehicles that stand still: points (n, m, d) -> the six tensors (pos0, pos1, pos2, vel1, duration0, duration1)
    of a fleet, with pos0 = pos1 = pos2 = points, all velocities 0 and both durations duration / 2 (they must be positive, or the NaN
    rule bites: duration must be finite and > 0).  Keep-out spheres as fleet B of trajectory_cross_contact.  The common domain of a
    pair ends at the smaller of its two vehicles' total times: an obstacle's duration must cover the window, or the queries are clamped
    to the obstacle's life.  Differentiable in points by composition."""
    who = "static_fleet"
    _check_is_tensor("points", points, who)
    if points.dim() != 3:
        raise ValueError("%s: points must have shape (n, m, d), got %s" % (who, tuple(points.shape)))
    _check_is_float64("points", points, who)
    duration = float(duration)
    if not (0.0 < duration < float("inf")):
        raise ValueError("%s: duration must be finite and positive, got %r" % (who, duration))
    half = torch.full(points.shape, 0.5 * duration, dtype=torch.float64, device=points.device)
    return [points, points, points, torch.zeros_like(half), half, half.clone()]


# What the two cross Functions share.  A vehicle of A owns a row of the (n, m_a, m_b, k) outputs and a vehicle of B a column: a side is the
# view of the pairs' arrays in which its vehicles' partners are contiguous, with the names _fleet_vjp and _route_end_bars read from
# _fleet_times -- tau, signs (+1 for A, the pair's first vehicle; -1 for B), through -- so every sum over partners is a reshape or permute
# and a sum.  back: a side's (n m, partners k) array as (n, pairs, k); spread: a value per vehicle, (n m,), as (n, pairs, 1).
_CrossSide = collections.namedtuple("_CrossSide", "tau signs through back spread")


def _cross_sides(m, t):
    """The two sides at the pairs' times t, (n, pairs, k) and contiguous, of m = (m_a, m_b) vehicles"""
    (m_a, m_b), (n, pairs, k) = m, t.shape
    one = torch.ones((1, 1, 1, 1), dtype=torch.float64, device=t.device)
    square = lambda x: x.reshape(n, m_a, m_b, -1)      # noqa: E731
    across = lambda x: square(x).permute(0, 2, 1, 3)      # noqa: E731
    side_a = _CrossSide(t.reshape(n * m_a, m_b * k).contiguous(), one, square, lambda x: x.reshape(n, pairs, k),
                        lambda x: x.reshape(n, m_a, 1, 1).expand(n, m_a, m_b, 1).reshape(n, pairs, 1))
    side_b = _CrossSide(across(t).reshape(n * m_b, m_a * k).contiguous(), -one, across,
                        lambda x: x.reshape(n, m_b, m_a, k).permute(0, 2, 1, 3).reshape(n, pairs, k),
                        lambda x: x.reshape(n, 1, m_b, 1).expand(n, m_a, m_b, 1).reshape(n, pairs, 1))
    return side_a, side_b


def _cross_setup(ctx, inputs, count, dead, outputs):
    """_fleet_setup for d, m_a, m_b in front: ctx.m is (m_a, m_b)"""
    ctx.d, ctx.m = inputs[0], (inputs[1], inputs[2])
    _keep(ctx, inputs[3:3 + count], outputs, dead)


def _cross_kept(ctx):
    """What _cross_setup kept: (A's and B's d lists of eight tensors, the other inputs among the `count`, the outputs)"""
    inputs, outputs = _kept(ctx)
    fleet_a, fleet_b = _axis_tables(inputs, ctx.d)
    return fleet_a, fleet_b, inputs[16 * ctx.d:], outputs


def _cross_gaps(fleets, sides):
    """The d gaps D_c at the pairs' times, (n, pairs, k) each: per axis one evaluator launch on A's n m_a splines and one on B's n m_b"""
    gaps = []
    for s_a, s_b in zip(*fleets):
        pos = []
        for s, side in zip((s_a, s_b), sides):
            out = _empty(side.tau.shape, side.tau.device)
            _enqueue(capi.trajectory_eval, side.tau.device, *side.tau.shape, s, side.tau, out, None, None)
            pos.append(side.back(out))
        gaps.append(pos[0] - pos[1])
    return gaps


def _cross_jvp(fleets, sides, gaps, dots, tau_dots):
    """Axis by axis, the evaluator's forward launch on each fleet's splines at its side's times; yields the axis' share of the tangent of
    the squared distance, 2 D_c (d pos_A,c - d pos_B,c), (n, pairs, k).  dots: A's 8 d tangents, then B's."""
    d = len(fleets[0])
    for c in range(d):
        pos_dot = []
        for v, side in enumerate(sides):
            out = _empty(side.tau.shape, side.tau.device)
            first = 8 * (v * d + c)
            _enqueue(capi.trajectory_eval_jvp, side.tau.device, *side.tau.shape, fleets[v][c], side.tau, dots[first:first + 8], tau_dots[v], out,
                     None, None)
            pos_dot.append(side.back(out))
        yield (2.0 * gaps[c]) * (pos_dot[0] - pos_dot[1])


def _cross_vjp(fleets, sides, need, want_tau, g_gap):
    """_fleet_vjp on both sides, axis by axis, A's launch before B's: yields (A's eight bars, B's, the pair's tau_bar shares (A's, B's) as
    (n, pairs, k), None unless want_tau)"""
    d = len(fleets[0])
    both = zip(_fleet_vjp(fleets[0], sides[0], need[:8 * d], want_tau, g_gap), _fleet_vjp(fleets[1], sides[1], need[8 * d:16 * d], want_tau, g_gap))
    for (bar_a, tau_a), (bar_b, tau_b) in both:
        yield bar_a, bar_b, ((sides[0].back(tau_a), sides[1].back(tau_b)) if want_tau else None)


class _TrajectoryCrossSeparation(torch.autograd.Function):
    """(sep_sq, t_closest), (n, pairs, k) each, of every vehicle of fleet A against every vehicle of fleet B over the scenes' windows.  Inputs:
    d, m_a, m_b, A's 8 d tensors, B's 8 d, lo, hi (n, k).  _TrajectoryFleetSeparation's derivatives with a row per vehicle of A and a column
    per vehicle of B where it has the slot table.  The time is not differentiable."""

    @staticmethod
    def forward(d, m_a, m_b, *inputs):
        lo, hi = (_dense(t) for t in inputs[16 * d:])
        given = lo if lo is not None else hi
        n = inputs[0].shape[0] // m_a
        k = given.shape[1] if given is not None else 1
        return _fleet_forward(capi.trajectory_cross_separation, d, (m_a, m_b), inputs, n, k, 2, lo, hi)

    @staticmethod
    def setup_context(ctx, inputs, output):
        _cross_setup(ctx, inputs, 16 * inputs[0] + 2, output[1:], output)

    @staticmethod
    def _saved(ctx):
        """(the two fleets' d lists of eight tensors; the two sides; where the value is NaN, (n, pairs, k); the d gaps D_c; the class masks
        LO, HI, [END of A's axis c], [END of B's], exclusive and in that priority)"""
        d = ctx.d
        fleet_a, fleet_b, (lo, hi), (value, time) = _cross_kept(ctx)
        missing = torch.isnan(value) | torch.isnan(time)
        t = torch.where(missing, torch.zeros_like(time), time)
        sides = _cross_sides(ctx.m, t)
        tests = [lo.unsqueeze(1) if lo is not None else None, hi.unsqueeze(1) if hi is not None else None]
        tests += [side.spread(s[6] + s[7]) for fleet, side in zip((fleet_a, fleet_b), sides) for s in fleet]
        masks = _class_masks(t, missing, tests)
        return (fleet_a, fleet_b), sides, missing, _cross_gaps((fleet_a, fleet_b), sides), (masks[0], masks[1], masks[2:2 + d], masks[2 + d:])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_value, _g_time):
        d = ctx.d
        if g_value is None:
            return (None,) * (16 * d + 5)
        fleets, sides, missing, gaps, (is_lo, is_hi, end_a, end_b) = _TrajectoryCrossSeparation._saved(ctx)
        g = torch.where(missing, torch.zeros_like(g_value), g_value)      # a NaN value: gradient 0
        need = ctx.needs_input_grad[3:]
        want_time = any(need[8 * c + 6] or need[8 * c + 7] for c in range(2 * d)) or any(need[16 * d:])
        # (a bad vehicle's gap is NaN: not into its partners)
        g_gap = lambda c: torch.where(missing, torch.zeros_like(g), (2.0 * g) * gaps[c])      # noqa: E731
        bars_a, bars_b, time_bar = [], [], None
        for bar_a, bar_b, shares in _cross_vjp(fleets, sides, need, want_time, g_gap):
            bars_a += bar_a
            bars_b += bar_b
            if want_time:      # the pair's: its two vehicles', added in _TrajectorySeparation's order
                for share in shares:
                    time_bar = share if time_bar is None else time_bar + share
        lo_bar = hi_bar = None
        if want_time:
            routed = lambda mask: torch.where(mask, time_bar, torch.zeros_like(time_bar))      # noqa: E731
            _route_end_bars(bars_a, need[:8 * d], sides[0], routed, end_a, end_b)
            _route_end_bars(bars_b, need[8 * d:16 * d], sides[1], routed, end_a, end_b)
            if need[16 * d]:
                lo_bar = routed(is_lo).sum(dim=1)
            if need[16 * d + 1]:
                hi_bar = routed(is_hi).sum(dim=1)
        return (None, None, None) + tuple(bars_a) + tuple(bars_b) + (lo_bar, hi_bar)

    @staticmethod
    def jvp(ctx, _t_d, _t_a, _t_b, *tangents):
        d = ctx.d
        fleets, sides, missing, gaps, (is_lo, is_hi, end_a, end_b) = _TrajectoryCrossSeparation._saved(ctx)
        dots = [_dense(t) for t in tangents[:16 * d]]
        zero = torch.zeros(missing.shape, dtype=torch.float64, device=missing.device)
        wide = lambda t: t.unsqueeze(1) if t is not None else zero      # noqa: E731
        time_dot = torch.where(is_lo, wide(tangents[16 * d]), zero)
        time_dot = torch.where(is_hi, wide(tangents[16 * d + 1]), time_dot)
        for v, ends in enumerate((end_a, end_b)):
            for c in range(d):
                total = None
                for t in (dots[8 * (v * d + c) + 6], dots[8 * (v * d + c) + 7]):
                    if t is not None:
                        total = t if total is None else total + t
                if total is not None:
                    time_dot = torch.where(ends[c], sides[v].spread(total), time_dot)
        tau_dots = [side.through(time_dot).reshape(side.tau.shape).contiguous() for side in sides]
        value_dot = zero
        for share in _cross_jvp(fleets, sides, gaps, dots, tau_dots):
            value_dot = value_dot + share
        return torch.where(missing, torch.full_like(zero, float("nan")), value_dot), None


class _TrajectoryCrossContact(torch.autograd.Function):
    """(time, rate), (n, pairs, k) each, of the first time in the scene's window at which the squared distance of a vehicle of A and one of B
    is at the level.  Inputs: d, m_a, m_b, A's 8 d tensors, B's 8 d, level_sq -- (n, k) or (n, pairs, k) --, lo, hi (n, k).
    _TrajectoryFleetContact's implicit-function formula with rows and columns for the slot table.  lo and hi only
    choose the branch.  rate is for the backward and is not differentiable."""

    @staticmethod
    def forward(d, m_a, m_b, *inputs):
        level, lo, hi = (_dense(t) for t in inputs[16 * d:])
        level, per_pair = _fleet_level(level)
        return _fleet_forward(capi.trajectory_cross_contact, d, (m_a, m_b), inputs, level.shape[0], level.shape[-1], 2, level, int(per_pair),
                              lo, hi)

    @staticmethod
    def setup_context(ctx, inputs, output):
        d = inputs[0]
        ctx.per_pair = inputs[3 + 16 * d].dim() == 3
        _cross_setup(ctx, inputs, 16 * d, output[1:], output)      # neither derivative reads the level, lo or hi

    @staticmethod
    def _saved(ctx):
        """(the two fleets' d lists of eight tensors; the two sides; rate; where there is no contact, (n, pairs, k); the d gaps D_c)"""
        fleet_a, fleet_b, _, (time, rate) = _cross_kept(ctx)
        missing = torch.isnan(time)
        sides = _cross_sides(ctx.m, torch.where(missing, torch.zeros_like(time), time))
        return (fleet_a, fleet_b), sides, rate, missing, _cross_gaps((fleet_a, fleet_b), sides)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_time, _g_rate):
        d = ctx.d
        if g_time is None:
            return (None,) * (16 * d + 6)
        fleets, sides, rate, missing, gaps = _TrajectoryCrossContact._saved(ctx)
        need = ctx.needs_input_grad[3:]
        zero = torch.zeros_like(rate)
        w = torch.where(missing, zero, g_time / rate)      # an unreached level: gradient 0
        # (a bad vehicle's gap is NaN: not into its partners)
        g_gap = lambda c: torch.where(missing, zero, -((2.0 * w) * gaps[c]))      # noqa: E731
        bars_a, bars_b = [], []
        for bar_a, bar_b, _ in _cross_vjp(fleets, sides, need, False, g_gap):
            bars_a += bar_a
            bars_b += bar_b
        level_bar = _level_bar(ctx, w) if need[16 * d] else None
        return (None, None, None) + tuple(bars_a) + tuple(bars_b) + (level_bar, None, None)

    @staticmethod
    def jvp(ctx, _t_d, _t_a, _t_b, *tangents):
        d = ctx.d
        fleets, sides, rate, missing, gaps = _TrajectoryCrossContact._saved(ctx)
        dots = [_dense(t) for t in tangents[:16 * d]]
        total = _level_dot(ctx, tangents[16 * d], rate)
        for share in _cross_jvp(fleets, sides, gaps, dots, (None, None)):
            total = total - share
        return torch.where(missing, torch.full_like(rate, float("nan")), total / rate), None


def _check_cross(fleet_a, fleet_b, who):
    """Two fleets as trajectory_cross_separation takes them, shapes and types: (n, m_a, m_b, d, A's d splines, B's)"""
    n, m_a, d, tables_a = _check_fleet(fleet_a, who, "fleet_a", _check_cross_size)
    n_b, m_b, d_b, tables_b = _check_fleet(fleet_b, who, "fleet_b", _check_cross_size)
    if n_b != n or d_b != d:
        raise ValueError("%s: fleet_a has %d scenes of %d axes, fleet_b %d of %d: the two fleets share their scenes and their axes"
                         % (who, n, d, n_b, d_b))
    return n, m_a, m_b, d, tables_a, tables_b


def _check_cross_devices(fleet_a, fleet_b, who):
    _check_fleet_devices(fleet_a, who)
    _check_fleet_devices(fleet_b, who)
    if fleet_b[0].device != fleet_a[0].device:
        raise TypeError("%s: fleet_b is on %s; it must be on fleet_a's device %s" % (who, fleet_b[0].device, fleet_a[0].device))


def _check_cross_queries(n, m_a, m_b, device, radius, level_sq, lo, hi, who):
    """_check_fleet_queries for the m_a m_b pairs of two fleets; a four-dimensional level (n, m_a, m_b, k) is the per-pair one's view."""
    given = radius if radius is not None else level_sq
    if isinstance(given, torch.Tensor) and given.dim() == 4:
        if tuple(given.shape[:3]) != (n, m_a, m_b) or given.shape[3] == 0:
            raise ValueError("%s: a four-dimensional %s must have shape (%d, %d, %d, k) -- one per vehicle of A and of B -- with k >= 1, got %s"
                             % (who, "radius" if radius is not None else "level_sq", n, m_a, m_b, tuple(given.shape)))
        given = given.reshape(n, m_a * m_b, given.shape[3])
        radius, level_sq = (given, None) if radius is not None else (None, given)
    name, level = _check_fleet_level(n, m_a * m_b, radius, level_sq, who)
    lo, hi = _check_fleet_windows(n, device, lo, hi, who)
    for other, t in (("lo", lo), ("hi", hi)):
        if t is not None and t.shape[1] != level.shape[-1]:
            raise ValueError("%s: %s has %d queries per scene, %s %d" % (who, name, level.shape[-1], other, t.shape[1]))
    if level.device != device:
        raise TypeError("%s: %s is on %s; it must be on the fleets' device %s" % (who, name, level.device, device))
    return level, lo, hi


def trajectory_cross_separation(fleet_a, fleet_b, lo=None, hi=None):
    """trajectory_separation for every vehicle of one fleet against every vehicle of another, in one launch: n scenes, in each m_a vehicles
    of fleet A and m_b of fleet B (1..32768 each) that move in d = 1, 2 or 3 axes, all on one clock -- your vehicles against the other
    team's, or against obstacles (static_fleet).  fleet_a, fleet_b: each a sequence of six tensors (pos0, pos1, pos2, vel1, duration0,
    duration1), or of eight with (vel0, vel2) appended, (n, m_a, d) and (n, m_b, d), float64 on one ROCm device.  lo, hi: exactly
    trajectory_fleet_separation's.  Returns (sep_sq, t_closest), (n, pairs, k) each, pairs = m_a m_b in cross_pairs(m_a, m_b)'s order,
    row-major -- reshape to (n, m_a, m_b, k): [s, (i, j), q] is bit for bit what trajectory_separation gives for vehicle i of A and vehicle
    j of B of scene s, the window [lo, hi][s, q] and no delay -- its NaN rule (a bad vehicle of A makes exactly its row NaN, one of B its
    column), domain, candidates and earliest-among-equals.  No pair within a fleet is looked at.

    One rp_trajectory_cross_separation launch on the current stream; no pair-expanded tensor is made.  sep_sq is differentiable to first
    order in all tensors of both fleets, lo and hi, in both modes: per axis and fleet one rp_trajectory_eval launch and one
    rp_trajectory_eval_vjp (reverse) or rp_trajectory_eval_jvp (forward) launch on the fleet's splines at the returned times (DESIGN.md
    section 34); a vehicle's sum over its partners is a reshape or permute and a sum, so a gradient is the same bits in every run; a double
    backward raises torch's once_differentiable error.  A NaN value has gradient 0 (forward mode: NaN).  The time is not differentiable.
    Does not synchronise the host."""
    who = "trajectory_cross_separation"
    n, m_a, m_b, d, tables_a, tables_b = _check_cross(fleet_a, fleet_b, who)
    lo, hi = _check_fleet_windows(n, fleet_a[0].device, lo, hi, who)
    _check_cross_devices(fleet_a, fleet_b, who)
    return _TrajectoryCrossSeparation.apply(d, m_a, m_b, *[t for table in tables_a + tables_b for t in table], lo, hi)


def trajectory_cross_contact(fleet_a, fleet_b, radius=None, lo=None, hi=None, *, level_sq=None):
    """trajectory_contact for every vehicle of one fleet against every vehicle of another, in one launch: the first time in a scene's
    windows [lo, hi] at which vehicle i of A and vehicle j of B come within `radius` of each other.  fleet_a, fleet_b, lo, hi: exactly
    trajectory_cross_separation's.  radius: (n, k), or (k,) for the same in every scene -- one radius for all pairs of a scene --, or
    (n, pairs, k) or (n, m_a, m_b, k) -- one per pair; the four-dimensional form is a view of the three-dimensional one, so
    (r_a[:, :, None, None] + r_b[:, None, :, None]).expand(n, m_a, m_b, k) is the call for vehicles and obstacles of different sizes.  The
    level is radius * radius, formed in torch, so the radius gets its gradient by the chain rule.  level_sq= may be given instead of
    radius (giving both, or neither, is a TypeError).  Returns t_contact, (n, pairs, k), pairs = m_a m_b in cross_pairs(m_a, m_b)'s order:
    [s, (i, j), q] is bit for bit what trajectory_contact gives for those two vehicles, the window [lo, hi][s, q], that query's level and
    no delay -- NaN where the pair does not reach the level in the window, and its NaN rule (rows and columns, as
    trajectory_cross_separation).  fleet_first_contact takes these times as they are: its index is then into cross_pairs(m_a, m_b).

    One rp_trajectory_cross_contact launch on the current stream.  Differentiable to first order in all tensors of both fleets and the
    level, in both modes, by trajectory_fleet_contact's formula with trajectory_cross_separation's launches and sums (DESIGN.md section
    34); lo and hi get no gradient; an unreached level has gradient 0 (forward mode: NaN).  Does not synchronise the host."""
    who = "trajectory_cross_contact"
    if (radius is None) == (level_sq is None):
        raise TypeError(who + ": give either radius or level_sq=, not %s" % ("both" if radius is not None else "neither"))
    n, m_a, m_b, d, tables_a, tables_b = _check_cross(fleet_a, fleet_b, who)
    level, lo, hi = _check_cross_queries(n, m_a, m_b, fleet_a[0].device, radius, level_sq, lo, hi, who)
    _check_cross_devices(fleet_a, fleet_b, who)
    return _TrajectoryCrossContact.apply(d, m_a, m_b, *[t for table in tables_a + tables_b for t in table], level, lo, hi)[0]


def _check_cross_problem(pos_a, pos_b, vel_a, vel_b, synchronize, who):
    """The two fleets of a cross pipeline, shapes and types: (n, m_a, m_b, d)"""
    n, m_a, d = _check_fleet_problem(pos_a, vel_a, synchronize, who, _check_cross_size)
    n_b, m_b, d_b = _check_fleet_problem(pos_b, vel_b, synchronize, who, _check_cross_size)
    if n_b != n or d_b != d:
        raise ValueError("%s: pos_a has %d scenes of %d axes, pos_b %d of %d: the two fleets share their scenes and their axes"
                         % (who, n, d, n_b, d_b))
    return n, m_a, m_b, d


def min_time_cross_separation(pos_a, pos_b, lo=None, hi=None, *, vel_a=None, vel_b=None, synchronize=True, gap_tol=1e-8, max_iter=200,
                              params=None):
    """min_time_solve of both fleets' axes, then trajectory_cross_separation of the solutions: min_time_fleet_separation's composition
    for two fleets.  pos_a, pos_b: (pos0, pos1, pos2), (n, m_a, d) and (n, m_b, d) each: the n (m_a + m_b) d axis problems are solved;
    vel_a, vel_b: (vel0, vel2) (None: rest to rest); synchronize (the default): each vehicle's axes are stretched to its slowest first.
    Returns (sep_sq, t_closest, solution_a, solution_b), the solutions as min_time_fleet_separation returns its.  Plain composition."""
    who = "min_time_cross_separation"
    n, m_a, m_b, d = _check_cross_problem(pos_a, pos_b, vel_a, vel_b, synchronize, who)
    lo, hi = _check_fleet_windows(n, pos_a[0].device, lo, hi, who)      # before the solves: a bad query costs none
    spline_a, solution_a = _solve_fleet(pos_a, vel_a, synchronize, gap_tol, max_iter, params)
    spline_b, solution_b = _solve_fleet(pos_b, vel_b, synchronize, gap_tol, max_iter, params)
    return tuple(trajectory_cross_separation(spline_a, spline_b, lo, hi)) + (solution_a, solution_b)


def min_time_cross_contact(pos_a, pos_b, radius=None, lo=None, hi=None, *, level_sq=None, vel_a=None, vel_b=None, synchronize=True,
                           gap_tol=1e-8, max_iter=200, params=None):
    """min_time_solve of both fleets' axes, then trajectory_cross_contact of the solutions: min_time_cross_separation's composition with
    trajectory_cross_contact's radius (or level_sq=), lo and hi.  Returns (t_contact, solution_a, solution_b)."""
    who = "min_time_cross_contact"
    if (radius is None) == (level_sq is None):
        raise TypeError(who + ": give either radius or level_sq=, not %s" % ("both" if radius is not None else "neither"))
    n, m_a, m_b, d = _check_cross_problem(pos_a, pos_b, vel_a, vel_b, synchronize, who)
    # before the solves: a bad query costs none
    level, lo, hi = _check_cross_queries(n, m_a, m_b, pos_a[0].device, radius, level_sq, lo, hi, who)
    spline_a, solution_a = _solve_fleet(pos_a, vel_a, synchronize, gap_tol, max_iter, params)
    spline_b, solution_b = _solve_fleet(pos_b, vel_b, synchronize, gap_tol, max_iter, params)
    return trajectory_cross_contact(spline_a, spline_b, None, lo, hi, level_sq=level), solution_a, solution_b


# ---- how much: integrals over a window ----
class _TrajectoryIntegrals(torch.autograd.Function):
    """(pos_int, distance, vel_sq, acc_sq) over the windows [lo, hi] clamped to the spline: differentiable to first order in the eight spline
    inputs (the table's order) and in lo and hi, each mode one launch of its own entry."""

    @staticmethod
    def forward(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, lo, hi):
        spline = [_dense(t) for t in (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1)]
        lo, hi = _dense(lo), _dense(hi)
        n, k = _query_shape(pos0.shape[0], lo, hi)
        outs = [_empty((n, k), pos0.device) for _ in range(4)]
        _enqueue(capi.trajectory_integrals, pos0.device, n, k, spline, lo, hi, outs)
        return tuple(outs)

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.shape = tuple(output[0].shape)
        _keep(ctx, inputs)

    @staticmethod
    def _inputs(ctx):
        inputs, _ = _kept(ctx)
        return [_dense(t) for t in inputs[:8]], _dense(inputs[8]), _dense(inputs[9])

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g):
        if all(x is None for x in g):
            return (None,) * 10
        spline, lo, hi = _TrajectoryIntegrals._inputs(ctx)
        return _integrals_vjp(spline, lo, hi, ctx.shape, g, ctx.needs_input_grad)

    @staticmethod
    def jvp(ctx, *tangents):
        spline, lo, hi = _TrajectoryIntegrals._inputs(ctx)
        dots = [_dense(t) for t in tangents]
        outs = [_empty(ctx.shape, spline[0].device) for _ in range(4)]
        _enqueue(capi.trajectory_integrals_jvp, spline[0].device, *ctx.shape, spline, lo, hi, dots[:8], dots[8], dots[9], outs)
        return tuple(outs)


def _integrals_vjp(spline, lo, hi, shape, g, need):
    """The one rp_trajectory_integrals_vjp launch of _TrajectoryIntegrals.backward and _IntegralsVJP.forward: the eight bars, lo_bar and
    hi_bar that `need` names, None for the others."""
    (n, k), dev = shape, spline[0].device
    bars = _bars(need[:8], n, dev)
    lo_bar, hi_bar = _bars(need[8:10], (n, k), dev)
    _enqueue(capi.trajectory_integrals_vjp, dev, n, k, spline, lo, hi, [_dense(x) for x in g], bars, lo_bar, hi_bar)
    return tuple(bars) + (lo_bar, hi_bar)


class _TrajectoryIntegrals2(_TrajectoryIntegrals):
    """_TrajectoryIntegrals with a backward that can be differentiated again (order=2): the same forward, the same forward-mode rule, and
    the same one rp_trajectory_integrals_vjp launch in backward, made through _IntegralsVJP so that a create_graph backward records it."""

    @staticmethod
    def backward(ctx, *g):
        return _backward2(ctx, _IntegralsVJP, g, ctx.shape)


class _IntegralsVJP(torch.autograd.Function):
    """(the eight spline inputs, lo, hi, the four upstream gradients) -> (the eight bars, lo_bar, hi_bar): one rp_trajectory_integrals_vjp
    launch that forms the bars `need` names (the others are None), as a function that can be differentiated once.  For cotangents u on
    its outputs:
        g_bar = J u                                                    one rp_trajectory_integrals_jvp launch with tangents u
        (spline, lo, hi)_bar = (S_o g_o (second derivative of o)) u    one rp_trajectory_integrals_hvp launch with direction u (symmetric)
    each made only if something on its side requires grad."""

    @staticmethod
    def forward(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, lo, hi, g0, g1, g2, g3, need, shape):
        spline = [_dense(t) for t in (pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1)]
        return _integrals_vjp(spline, _dense(lo), _dense(hi), shape, (g0, g1, g2, g3), need)

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.shape = tuple(inputs[15])
        _keep(ctx, inputs[:14], forward=False)      # (a bar nothing downstream uses arrives as None too)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *u):
        out = [None] * 16
        if all(x is None for x in u):
            return tuple(out)
        inputs, _ = _kept(ctx)
        spline, lo, hi, g = [_dense(t) for t in inputs[:8]], _dense(inputs[8]), _dense(inputs[9]), [_dense(t) for t in inputs[10:14]]
        need, (n, k), dev = ctx.needs_input_grad, ctx.shape, spline[0].device
        dots, lo_dot, hi_dot = [_dense(x) for x in u[:8]], _dense(u[8]), _dense(u[9])
        if any(need[10:14]):
            outs = _bars(need[10:14], (n, k), dev)
            _enqueue(capi.trajectory_integrals_jvp, dev, n, k, spline, lo, hi, dots, lo_dot, hi_dot, outs)
            out[10:14] = outs
        if any(need[:10]) and any(x is not None for x in g):
            bars = _bars(need[:8], n, dev)
            lo_bar, hi_bar = _bars(need[8:10], (n, k), dev)
            _enqueue(capi.trajectory_integrals_hvp, dev, n, k, spline, lo, hi, g, dots, lo_dot, hi_dot, bars, lo_bar, hi_bar)
            out[:10] = bars + [lo_bar, hi_bar]
        return tuple(out)


def trajectory_integrals(pos0, pos1, pos2, vel1, duration0, duration1, lo=None, hi=None, *, vel0=None, vel2=None, order=1):
    """The integrals of the spline of trajectory_eval over the windows of time [lo, hi] -- (n, k), or (k,) for the same windows in every
    problem; None: -inf / +inf, both None: k = 1, the whole spline -- clamped to [0, duration0 + duration1] (no extrapolation).  Returns
    (pos_int, distance, vel_sq, acc_sq), (n, k) each: the integrals of pos, |vel| (the distance actually travelled), vel^2 and acc^2.  NaN
    where the clamped window is empty (a NaN end, a window wholly outside the spline); exactly 0 where its ends coincide.

    One rp_trajectory_integrals launch on the current stream (include/rp_batch.h: closed forms in the segment constants, the window split
    at the knot and, for the distance, at the roots of the velocity).  Differentiable to first order in all eight spline inputs and in lo
    and hi: reverse mode is one rp_trajectory_integrals_vjp launch that forms only the gradients autograd asks for, forward mode
    (torch.autograd.forward_ad, torch.func.jvp) one rp_trajectory_integrals_jvp launch; a double backward raises
    torch's once_differentiable error.  Where a window end is clamped, and at ties (an end on the knot), the derivative is that of the
    branch the forward pass took.  A NaN output has gradient 0 (forward mode: NaN).  Does not synchronise the host.

    order=2 (1 or 2; anything else: ValueError) makes the backward differentiable once more -- torch.autograd.grad(..., create_graph=True),
    torch.autograd.functional.hvp / hessian: the values, the gradients and the forward-mode tangents are the same launches and the same
    bits as with order=1; the backward of the backward is one rp_trajectory_integrals_jvp launch (for the gradients in the first
    backward's grad_outputs) and one rp_trajectory_integrals_hvp launch (for those in the spline inputs, lo and hi), each only if something
    on its side requires grad.  The second derivative is that of the branch the forward took; the distance's has a
    term at every sign change of the velocity inside the window, large near a double root.  A third derivative raises torch's
    once_differentiable error."""
    who = "trajectory_integrals"
    _check_order(order, who)
    _check_trajectory(pos0, pos1, pos2, vel1, duration0, duration1, None, vel0, vel2, who, None)
    lo, hi = _check_window(pos0, lo, hi, who)
    function = _TrajectoryIntegrals if order == 1 else _TrajectoryIntegrals2
    return function.apply(pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1, lo, hi)


def min_time_integrals(pos0, pos1, pos2, lo=None, hi=None, *, vel0=None, vel2=None, gap_tol=1e-8, max_iter=200, params=None, order=1):
    """min_time_solve, then trajectory_integrals of its solution over [lo, hi] ((n, k), (k,) or None): returns the four of
    trajectory_integrals, then (vel1, duration0, duration1, iters, status).  Plain composition: the integrals are differentiable in the
    positions, the end velocities and the window's ends through the solve's derivatives and the integrals'.

    order=2 (trajectory_integrals'): with the solve's own double backward, the integrals are twice differentiable in the positions and the
    window's ends for rest-to-rest problems.  With vel0 / vel2 that require grad the solve is first order, and a double backward through
    it raises torch's once_differentiable error as it does with order=1."""
    _check_order(order, "min_time_integrals")
    _check_positions(pos0, pos1, pos2, "min_time_integrals")
    lo, hi = _check_window(pos0, lo, hi, "min_time_integrals")      # before the solve: a bad window costs none
    vel1, duration0, duration1, iters, status = min_time_solve(pos0, pos1, pos2, gap_tol=gap_tol, max_iter=max_iter, params=params,
                                                                vel0=vel0, vel2=vel2)
    out = trajectory_integrals(pos0, pos1, pos2, vel1, duration0, duration1, lo, hi, vel0=vel0, vel2=vel2, order=order)
    return tuple(out) + (vel1, duration0, duration1, iters, status)


# ---- how far apart two splines are on average: the tracking integrals over a window ----
class _TrajectoryTracking(torch.autograd.Function):
    """(gap_int, gap_sq, relvel_sq) of D(t) = pos_A(t) - pos_B(t - delay) over the windows [lo, hi] clamped to the two splines' common domain:
    differentiable to first order in the sixteen spline inputs (A's table, then B's), in lo, hi and the delay, each mode one call of its own
    entry."""

    @staticmethod
    def forward(*inputs):
        a, b = [_dense(t) for t in inputs[:8]], [_dense(t) for t in inputs[8:16]]
        lo, hi, delay = (_dense(t) for t in inputs[16:19])
        n, k = _query_shape(inputs[0].shape[0], lo, hi, delay)
        outs = [_empty((n, k), inputs[0].device) for _ in range(3)]
        _enqueue(capi.trajectory_tracking, inputs[0].device, n, k, a, b, lo, hi, delay, outs)
        return tuple(outs)

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.shape = tuple(output[0].shape)
        _keep(ctx, inputs)

    @staticmethod
    def _inputs(ctx):
        inputs = [_dense(t) for t in _kept(ctx)[0]]
        return inputs[:8], inputs[8:16], inputs[16], inputs[17], inputs[18]

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *g):
        if all(x is None for x in g):
            return (None,) * 19
        return _tracking_vjp(*_TrajectoryTracking._inputs(ctx), ctx.shape, g, ctx.needs_input_grad)

    @staticmethod
    def jvp(ctx, *tangents):
        a, b, lo, hi, delay = _TrajectoryTracking._inputs(ctx)
        dots = [_dense(t) for t in tangents]
        outs = [_empty(ctx.shape, a[0].device) for _ in range(3)]
        _enqueue(capi.trajectory_tracking_jvp, a[0].device, *ctx.shape, a, b, lo, hi, delay, dots[:8], dots[8:16], dots[16], dots[17], dots[18],
                 outs)
        return tuple(outs)


def _tracking_vjp(a, b, lo, hi, delay, shape, g, need):
    """The one rp_trajectory_tracking_vjp call of _TrajectoryTracking.backward and _TrackingVJP.forward: the sixteen bars, lo_bar, hi_bar
    and delay_bar that `need` names, None for the others."""
    (n, k), dev = shape, a[0].device
    bars = _bars(need[:16], n, dev)
    per_query = _bars(need[16:19], (n, k), dev)
    if any(need[:19]):
        _enqueue(capi.trajectory_tracking_vjp, dev, n, k, a, b, lo, hi, delay, [_dense(x) for x in g], bars[:8], bars[8:], *per_query)
    return tuple(bars) + tuple(per_query)


class _TrajectoryTracking2(_TrajectoryTracking):
    """_TrajectoryTracking with a backward that can be differentiated again (order=2): the same forward, the same forward-mode rule, and
    the same one rp_trajectory_tracking_vjp call in backward, made through _TrackingVJP so that a create_graph backward records it."""

    @staticmethod
    def backward(ctx, *g):
        return _backward2(ctx, _TrackingVJP, g, ctx.shape)


class _TrackingVJP(torch.autograd.Function):
    """(the sixteen spline inputs, lo, hi, delay, the three upstream gradients) -> (the sixteen bars, lo_bar, hi_bar, delay_bar): one
    rp_trajectory_tracking_vjp call that forms the bars `need` names (the others are None), as a function that can be differentiated once.
    For cotangents u on its outputs:
        g_bar = J u                                                  one rp_trajectory_tracking_jvp launch with tangents u
        (splines, lo, hi, delay)_bar = (S_o g_o (second derivative of o)) u
                                                                     one rp_trajectory_tracking_hvp call with direction u (symmetric)
    each made only if something on its side requires grad."""

    @staticmethod
    def forward(*inputs):
        need, shape = inputs[22], inputs[23]
        a, b = [_dense(t) for t in inputs[:8]], [_dense(t) for t in inputs[8:16]]
        lo, hi, delay = (_dense(t) for t in inputs[16:19])
        return _tracking_vjp(a, b, lo, hi, delay, shape, inputs[19:22], need)

    @staticmethod
    def setup_context(ctx, inputs, output):
        ctx.shape = tuple(inputs[23])
        _keep(ctx, inputs[:22], forward=False)      # (a bar nothing downstream uses arrives as None too)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, *u):
        out = [None] * 24
        if all(x is None for x in u):
            return tuple(out)
        inputs = [_dense(t) for t in _kept(ctx)[0]]
        a, b, (lo, hi, delay), g = inputs[:8], inputs[8:16], inputs[16:19], inputs[19:22]
        need, (n, k), dev = ctx.needs_input_grad, ctx.shape, a[0].device
        dots = [_dense(x) for x in u]
        if any(need[19:22]):
            outs = _bars(need[19:22], (n, k), dev)
            _enqueue(capi.trajectory_tracking_jvp, dev, n, k, a, b, lo, hi, delay, dots[:8], dots[8:16], dots[16], dots[17], dots[18], outs)
            out[19:22] = outs
        if any(need[:19]) and any(x is not None for x in g):
            bars = _bars(need[:16], n, dev)
            per_query = _bars(need[16:19], (n, k), dev)
            _enqueue(capi.trajectory_tracking_hvp, dev, n, k, a, b, lo, hi, delay, g, dots[:8], dots[8:16], dots[16], dots[17], dots[18],
                     bars[:8], bars[8:], *per_query)
            out[:19] = bars + per_query
        return tuple(out)


def trajectory_tracking(a, b, lo=None, hi=None, delay=None, *, order=1):
    """The tracking integrals between two splines of trajectory_eval in one frame: with D(t) = pos_a(t) - pos_b(t - delay), the integrals of
    D (gap_int), D^2 (gap_sq) and (dD/dt)^2 (relvel_sq) over the windows of time [lo, hi].  a, b, lo, hi, delay: exactly trajectory_gap's
    -- each spline a sequence of six tensors (pos0, pos1, pos2, vel1, duration0, duration1), or of eight with (vel0, vel2) appended, of the
    same n on the same ROCm device; the queries (n, k), or (k,) for the same queries in every problem; None: -inf / +inf / 0, all three
    None: k = 1, the whole common domain.  No extrapolation: the window is clamped to [max(delay, 0), min(T_a, delay + T_b)].  Returns
    (gap_int, gap_sq, relvel_sq), (n, k) each; NaN where the clamped window is empty, where the delay is NaN or infinite, and for a problem
    either of whose splines has a duration that is not finite or not > 0; exactly 0 where the window's ends coincide.  The mean gap over a
    window is gap_int / (b - a), the RMS gap sqrt(gap_sq / (b - a)).

    One rp_trajectory_tracking launch on the current stream (include/rp_batch.h: closed forms on the at most three pieces the two knots cut
    the window into).  Differentiable to first order in all sixteen spline inputs, lo, hi and delay: reverse mode is one
    rp_trajectory_tracking_vjp call that forms only the gradients autograd asks for, forward mode (torch.autograd.forward_ad,
    torch.func.jvp) one rp_trajectory_tracking_jvp launch; a double backward raises torch's once_differentiable
    error.  Where a window end is clamped, and at ties, the derivative is that of the branch the forward pass took; at a delay of exactly 0
    the clamped start is the constant +0.0.  A NaN output has gradient 0 (forward mode: NaN).  Does not synchronise the host.

    order=2 (1 or 2; anything else: ValueError) makes the backward differentiable once more -- torch.autograd.grad(..., create_graph=True),
    torch.autograd.functional.vhp / hessian: the values, the gradients and the forward-mode tangents are the same launches and the same
    bits as with order=1; the backward of the backward is one rp_trajectory_tracking_jvp launch (for the gradients in the first backward's
    grad_outputs) and one rp_trajectory_tracking_hvp call (for those in the spline inputs, lo, hi and delay), each only if something on its
    side requires grad.  The second derivative is that of the branch the forward took: exact, one-sided at ties and
    at a delay of exactly 0.  A third derivative raises torch's once_differentiable error.  (torch.autograd.functional.hvp runs but forms
    its product by differentiating the double backward in its own cotangent, which a once-differentiable backward does not offer, and
    reports zeros: the matrix is symmetric, so functional.vhp, which is the double backward, gives the same product.)"""
    who = "trajectory_tracking"
    _check_order(order, who)
    _check_spline_arg("a", a, who)
    _check_spline_arg("b", b, who)
    table_a, table_b = _spline_table("a", a, who), _spline_table("b", b, who)
    _check_same_batch(table_a[0], table_b[0], who)
    lo, hi, delay = _check_gap_queries(table_a[0], lo, hi, delay, who)
    function = _TrajectoryTracking if order == 1 else _TrajectoryTracking2
    return function.apply(*table_a, *table_b, lo, hi, delay)


def min_time_tracking(pos_a, pos_b, lo=None, hi=None, delay=None, *, vel_a=None, vel_b=None, gap_tol=1e-8, max_iter=200, params=None,
                      order=1):
    """min_time_solve of two vehicles' problems, then trajectory_tracking of the two solutions.  Arguments as min_time_gap's.  Returns
    (gap_int, gap_sq, relvel_sq, solution_a, solution_b) with each solution min_time_solve's (vel1, duration0, duration1, iters, status).
    Plain composition: the integrals are differentiable to first order in both vehicles' positions and end velocities, in lo, hi and delay,
    in both modes, through the solves' derivatives and the integrals'.

    order=2 (trajectory_tracking's): with the solves' own double backward, the integrals are twice differentiable in both vehicles'
    positions, the window's ends and the delay for rest-to-rest problems.  With vel_a / vel_b that require grad the solve is first order,
    and a double backward through it raises torch's once_differentiable error as it does with order=1."""
    who = "min_time_tracking"
    _check_order(order, who)
    _check_vehicles(pos_a, pos_b, vel_a, vel_b, who)
    lo, hi, delay = _check_gap_queries(pos_a[0], lo, hi, delay, who)      # before the solves: a bad query costs none
    splines, solutions = _solve_vehicles(pos_a, pos_b, vel_a, vel_b, gap_tol, max_iter, params)
    return tuple(trajectory_tracking(splines[0], splines[1], lo, hi, delay, order=order)) + (solutions[0], solutions[1])


def clear_pool():
    """Release every pooled batch that no autograd graph holds (device memory back to the allocator)."""
    _pool.clear()
