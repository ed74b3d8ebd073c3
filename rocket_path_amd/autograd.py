"""Torch layer over the batched F3 solve: tensors in, tensors out on the current stream, differentiable in the positions.

    vel1, duration0, duration1, iters, status = min_time_solve(pos0, pos1, pos2)
    (duration0 + duration1).sum().backward()      # -> pos0.grad, pos1.grad, pos2.grad

The forward is Batch.set_problems_device + the fused gated solve + Batch.solution_device into a torch buffer, enqueued without
synchronising the host.  The backward is one rp_batch_solution_vjp launch at the state the forward left (include/rp_batch.h,
DESIGN.md section 12): the implicit-function derivative of the central-path point the solve stopped at.  F3, float64 only; no
double backward.
"""
import ctypes
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


def _check_positions(pos0, pos1, pos2):
    for name, t in (("pos0", pos0), ("pos1", pos1), ("pos2", pos2)):
        if not isinstance(t, torch.Tensor):
            raise TypeError("min_time_solve: %s must be a torch.Tensor, got %s" % (name, type(t).__name__))
        if t.device.type != "cuda":
            raise TypeError("min_time_solve: %s is on %s; the solve runs on a ROCm device only (move it with .cuda())" % (name, t.device))
        if t.dtype != torch.float64:
            raise TypeError("min_time_solve: %s has dtype %s; float64 is required" % (name, t.dtype))
        if t.dim() != 1:
            raise ValueError("min_time_solve: %s must be 1-D, got shape %s" % (name, tuple(t.shape)))
    if not (pos0.shape == pos1.shape == pos2.shape):
        raise ValueError("min_time_solve: lengths differ (%d, %d, %d)" % (pos0.shape[0], pos1.shape[0], pos2.shape[0]))
    if not (pos0.device == pos1.device == pos2.device):
        raise ValueError("min_time_solve: positions on different devices (%s, %s, %s)" % (pos0.device, pos1.device, pos2.device))
    if pos0.shape[0] == 0:
        raise ValueError("min_time_solve: empty batch")


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


class _MinTimeSolve(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos0, pos1, pos2, gap_tol, max_iter, params, keep):
        device = pos0.device.index if pos0.device.index is not None else torch.cuda.current_device()
        n = pos0.shape[0]
        cur = torch.cuda.current_stream(device)
        handle = _stream_handle(cur)
        key = (device, n, handle)
        batch = _pool.take(key)
        # the null stream cannot be handed to a batch (NULL = "create your own"): then the batch's own stream is ordered by events
        ext = None if handle else torch.cuda.ExternalStream(batch.stream(), device=pos0.device)
        p0, p1, p2 = (t.contiguous() for t in (pos0, pos1, pos2))
        out = torch.empty((n, 4), dtype=torch.float64, device=pos0.device)      # n rp_solution records (torch's blocks: 512-byte aligned)
        try:
            p = capi.Params()
            batch._lib.rp_params_default(ctypes.byref(p))
            for k, v in (params or {}).items():
                setattr(p, k, v)
            capi.check(batch._lib.rp_batch_set_params(batch._h, ctypes.byref(p)))
            with _run_on(ext, cur):
                batch.set_problems_device(p0.data_ptr(), p1.data_ptr(), p2.data_ptr())
                batch.solve(gap_tol, max_iter, 0)
                batch.solution_device(out.data_ptr())
            if ext is not None:
                for t in (p0, p1, p2, out):
                    t.record_stream(ext)
        except Exception:
            _pool.give(key, batch)
            raise
        vel1, dur0, dur1 = out[:, 0].clone(), out[:, 1].clone(), out[:, 2].clone()
        words = out.view(torch.int32).view(n, 8)
        iters, status = words[:, 6].clone(), words[:, 7].clone()
        ctx.mark_non_differentiable(iters, status)
        if keep:
            ctx.lease = _Lease(key, batch)      # held by the graph until it is freed: its state is what the backward differentiates
            ctx.device = pos0.device
        else:
            _pool.give(key, batch)      # the read-back is enqueued; the next user of this key works on the same stream
        return vel1, dur0, dur1, iters, status

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_vel1, g_dur0, g_dur1, _g_iters, _g_status):
        batch = ctx.lease.batch
        device = ctx.device
        cur = torch.cuda.current_stream(device)
        bstream = torch.cuda.ExternalStream(batch.stream(), device=device)
        gs = [g.contiguous() if g is not None else None for g in (g_vel1, g_dur0, g_dur1)]
        n = batch.n
        bars = [torch.empty(n, dtype=torch.float64, device=device) for _ in range(3)]
        same = bstream.cuda_stream == cur.cuda_stream
        with _run_on(None if same else bstream, cur):
            batch.solution_vjp(*[g.data_ptr() if g is not None else 0 for g in gs], *[b.data_ptr() for b in bars])
        if not same:
            for t in gs + bars:
                if t is not None:
                    t.record_stream(bstream)
        return bars[0], bars[1], bars[2], None, None, None, None


def min_time_solve(pos0, pos1, pos2, *, gap_tol=1e-8, max_iter=200, params=None):
    """Solve the F3 problems (pos0[i], pos1[i], pos2[i]) -- 1-D float64 tensors on one ROCm device -- on the current stream.

    Returns (vel1, duration0, duration1, iters, status): float64 tensors, differentiable with respect to the positions, and the
    int32 step counts and RP_ST_* status words (not differentiable).  `params`: rp_params fields to override (a dict).
    Gradients are the implicit-function derivative at the state the solve returns (include/rp_batch.h, rp_batch_solution_vjp):
    NaN for problems whose state is not finite or not strictly feasible.  Does not synchronise the host."""
    _check_positions(pos0, pos1, pos2)
    if params is not None:
        unknown = set(params) - _PARAM_FIELDS
        if unknown:
            raise ValueError("min_time_solve: unknown rp_params field(s) %s" % sorted(unknown))
    keep = torch.is_grad_enabled() and any(t.requires_grad for t in (pos0, pos1, pos2))      # (forward itself runs with grad off)
    return _MinTimeSolve.apply(pos0, pos1, pos2, float(gap_tol), int(max_iter), params, keep)


def clear_pool():
    """Release every pooled batch that no autograd graph holds (device memory back to the allocator)."""
    _pool.clear()
