"""A/B of the torch layer of the spline and pair queries (rocket_path_amd/autograd.py) between two source trees that
load the same librp_batch.so: the same bits in every output, gradient and tangent, and the same host cost.  The loader, the SHA-1 compare
and the alternating timer are profiles/fleet_refactor_ab.py's.  Modes, each a fresh process:

    python profiles/query_refactor_ab.py bits OUT.npz [TREE]      every output, gradient, tangent and double-backward result into one file
    python profiles/query_refactor_ab.py compare A.npz B.npz      per-array SHA-1 of two such files; exit status 1 unless all are equal
    python profiles/query_refactor_ab.py time PARENT_TREE [NEW_TREE]   forward + backward per public function, the trees alternating
    python profiles/query_refactor_ab.py time-one [TREE]          one side's medians (what `time` starts, each with its own time limit)

bits: trajectory_eval, _crossing, _extrema, _integrals, _gap, _meeting, _tracking, _separation and _contact and their min_time_*
compositions; order=2 of the three families that have it.  n = 5, k = 1 and 4, d = 1, 2, 3 for separation and contact; end velocities
given and None; every optional query argument given and None.  Per call: every output; the reverse-mode gradients with every input
requiring grad and all differentiable outputs used, and again with only the query arguments requiring grad and only the first output
used; the forward-mode tangents (torch.autograd.forward_ad) with a tangent on every input and with tangents on the query arguments only,
and once more through torch.func.jvp; with order=2 the double backward in the inputs and in the first backward's grad_outputs.  The
problems are hand-made in dyadic numbers (tests/extrema_ref.py and tests/gap_ref.py have the reasoning for the knot cases): one problem
has a NaN duration, one window lies wholly outside the spline, one level is not reached, one window has zero width (class LO), one ends
past the spline (END), one ends on duration0; the two-spline problems have a positive delay with the extreme at the delayed start (START)
and at B's end (END_B).  How many times fall into each class is printed; exit status 3 if a class stayed empty, 4 if a call refused its
arguments (the message is kept as an array, so that both sides have to refuse alike; any other error ends the run).

time: n = 5, k = 4, d = 3, everything requiring a gradient; per function the median wall-clock time, host synchronised, of forward plus
backward -- the timer and its verdict (the new median within the parent's own spread across rounds) are fleet_refactor_ab.timing's."""
import json
import os
import sys
import time as clock

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import fleet_refactor_ab as ab      # noqa: E402

DEV = ab.DEV
N = 5
NAN, INF = float("nan"), float("inf")

# one spline: pos0, pos1, pos2, vel0, vel2, vel1, duration0, duration1 (the C ABI's table order)
SINGLE = [
    (0.0, 1.0, 2.0, 0.0, 0.0, 1.625, 1.0, 1.0),            # rises; acc changes sign across the knot: vel has its kink maximum there
    (0.25, -0.5, 0.75, 0.0, 0.0, 0.25, NAN, 1.25),         # a NaN duration
    (0.25, -0.5, 0.75, 0.125, -0.25, 0.25, 0.75, 1.25),    # turns round: interior extremes
    (2.0, 1.0, 0.0, 0.0, 0.0, -1.625, 1.0, 1.0),           # falls
    (-1.0, 0.5, 0.25, 0.0, 0.0, 0.5, 1.25, 0.75),
]
# two splines in one frame: A, B, delay -- gap_ref.knot_cases' KNOT_A, KNOT_B and END_B, then END_A with START, then a NaN duration
PAIRS = [
    ((0.0, 4.0, 16.0, 0.0, 16.0, 8.0, 1.0, 1.0), (0.0, 16.0, 24.0, 8.0, 8.0, 8.0, 2.0, 1.0), -0.5),
    ((0.0, 8.0, 16.0, 8.0, 8.0, 8.0, 1.0, 1.0), (0.0, 4.0, 16.0, 0.0, 16.0, 8.0, 1.0, 1.0), 0.25),
    ((0.0, 64.0, 128.0, 0.0, 0.0, 48.0, 2.0, 2.0), (0.0, -50.0, -100.0, 0.0, 0.0, -75.0, 1.0, 1.0), 0.5),
    ((0.0, 1.0, 2.0, 0.0, 0.0, 1.625, 1.0, 1.0), (5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.5, 1.5), 0.5),
    ((0.0, -50.0, -100.0, 0.0, 0.0, -75.0, NAN, 1.0), (0.0, 100.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0), 0.5),
]
# two vehicles, axis 0 (axis c is the same motion scaled by 1 + c / 4 and shifted by c / 8): moving apart from the delayed START; closing
# in until B's end; until A's end; a NaN duration; passing each other (a stationary point inside)
VEHICLES = [
    ((0.0, -1.0, -2.0, 0.0, 0.0, -1.625, 1.0, 1.0), (5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.0, 1.0), 0.5),
    ((0.0, 1.0, 2.0, 0.0, 0.0, 0.8125, 2.0, 2.0), (5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 0.75, 0.75), 0.5),
    ((0.0, 1.0, 2.0, 0.0, 0.0, 1.625, 1.0, 1.0), (5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.5, 1.5), 0.5),
    ((0.0, 1.0, 2.0, 0.0, 0.0, 1.625, 1.0, NAN), (5.0, 5.0, 5.0, 0.0, 0.0, 0.0, 1.5, 1.5), 0.5),
    ((0.0, 1.0, 2.0, 0.0, 0.0, 1.625, 1.0, 1.0), (2.0, 1.0, 0.0, 0.0, 0.0, -1.625, 1.0, 1.0), 0.25),
]


def table(torch, rows):
    """The eight (n,) tensors of `rows`, in the table's order"""
    return [torch.tensor([r[f] for r in rows], dtype=torch.float64, device=DEV) for f in range(8)]


def public(t, vel):
    """A table as the public functions take a spline: (pos0, pos1, pos2, vel1, duration0, duration1), and [vel0, vel2] or [None, None]"""
    return [t[0], t[1], t[2], t[5], t[6], t[7]], ([t[3], t[4]] if vel else [None, None])


def columns(torch, x, k):
    """x (n, 4) as it is, or for k = 1 one column: problem i keeps its query i mod 4"""
    if k == 4:
        return x
    return x.gather(1, (torch.arange(x.shape[0], device=x.device) % 4).unsqueeze(1))


def windows(torch, k, knot, outside, early=0.0):
    """lo, hi (n, k): a window of zero width; one that ends past the spline; one that ends on `knot` (n,); one inside -- which lies wholly
    outside the spline for problem `outside`.  early: by how much the finite ends come before 1, 0.75 and [1.25, 1.75]"""
    n = knot.shape[0]
    lo = torch.tensor([[1.0 - early, -9.0, 0.75 - early, 1.25 - early]] * n, dtype=torch.float64, device=DEV)
    hi = torch.tensor([[1.0 - early, 9.0, 0.0, 1.75 - early]] * n, dtype=torch.float64, device=DEV)
    hi[:, 2] = knot
    lo[outside, 3], hi[outside, 3] = 100.0, 101.0
    return columns(torch, lo, k), columns(torch, hi, k)


class Recorder(ab.Recorder):
    def __init__(self, torch):
        super().__init__(torch)
        self.errors = []

    def sort(self, who, time, missing, tests, last_only=None):
        """Counts the times by class as autograd._class_masks sorts them: tests are (name, reference or None), exclusive in that order"""
        taken = missing
        for at, (name, ref) in enumerate(tests):
            mask = (time == ref) & ~taken if ref is not None else self.torch.zeros_like(missing)
            if last_only is not None and at == len(tests) - 1:
                mask = mask & last_only
            self.count("%s: %s" % (who, name), mask)
            taken = taken | mask
        self.count("%s: elsewhere" % who, ~taken)
        self.count("%s: no value" % who, missing)

    def reached(self, who, time):
        self.count("%s: reached" % who, ~self.torch.isnan(time))
        self.count("%s: not reached" % who, self.torch.isnan(time))

    def record(self, name, function, inputs, diff, queries, second=False):
        """function(*inputs) -> a tuple of tensors, the first `diff` differentiable; inputs may hold None; queries: the places of the
        per-query arguments.  Returns the detached outputs, or None if the call raised."""
        try:
            return self._record(name, function, inputs, diff, queries, second)
        except (TypeError, ValueError, IndexError, KeyError, AttributeError, NotImplementedError) as e:      # kept: the other side has to raise the same
            text = "%s: %s" % (type(e).__name__, e)
            self.errors.append("%s -> %s" % (name, text))
            self.arrays[name.replace("/", " | ") + " | raised"] = __import__("numpy").frombuffer(text.encode(), dtype="uint8")
            return None

    def _record(self, name, function, inputs, diff, queries, second):
        torch = self.torch
        import torch.autograd.forward_ad as fwAD
        g = torch.Generator().manual_seed(len(self.arrays))
        seeded = lambda t: torch.randn(t.shape, dtype=torch.float64, generator=g).to(DEV)      # noqa: E731
        kept = None
        for tag, which in (("all", range(len(inputs))), ("queries", queries)):
            leaves = [t.detach().clone().requires_grad_(j in which) if t is not None else None for j, t in enumerate(inputs)]
            out = function(*leaves)
            if tag == "all":
                kept = [o.detach() for o in out]
                for j, o in enumerate(out):
                    self.keep("%s/out %d" % (name, j), o)
            used = list(out[:diff]) if tag == "all" else [out[0]]
            wanted = [(j, t) for j, t in enumerate(leaves) if t is not None and t.requires_grad]
            if not wanted:
                continue
            cots = [seeded(o).requires_grad_(second) for o in used]
            grads = torch.autograd.grad(used, [t for _, t in wanted], grad_outputs=cots, allow_unused=True, create_graph=second)
            for (j, _), x in zip(wanted, grads):
                self.keep("%s/%s bar %d" % (name, tag, j), x)
            live = [x for x in grads if x is not None and x.requires_grad] if second else []
            if live:
                total = sum((x * seeded(x)).sum() for x in live)
                again = torch.autograd.grad(total, [t for _, t in wanted] + cots, allow_unused=True)
                for j, x in enumerate(again):
                    self.keep("%s/%s bar bar %d" % (name, tag, j), x)
        for tag, which in (("all", range(len(inputs))), ("queries", queries)):
            with fwAD.dual_level():
                duals = [(fwAD.make_dual(t.detach(), seeded(t)) if j in which else t.detach()) if t is not None else None
                         for j, t in enumerate(inputs)]
                out = function(*duals)
                for j in range(diff):
                    self.keep("%s/%s dot %d" % (name, tag, j), fwAD.unpack_dual(out[j]).tangent)
        given = [j for j, t in enumerate(inputs) if t is not None]

        def closed(*xs):
            full = [None] * len(inputs)
            for j, x in zip(given, xs):
                full[j] = x
            return tuple(function(*full)[:diff])
        try:
            _, dots = torch.func.jvp(closed, tuple(inputs[j].detach() for j in given), tuple(seeded(inputs[j]) for j in given))
            for j, x in enumerate(dots):
                self.keep("%s/func dot %d" % (name, j), x)
        except (TypeError, ValueError, NotImplementedError) as e:
            text = "%s: %s" % (type(e).__name__, e)
            self.errors.append("%s (torch.func.jvp) -> %s" % (name, text))
            self.arrays[name.replace("/", " | ") + " | func raised"] = __import__("numpy").frombuffer(text.encode(), dtype="uint8")
        return kept


def subsets(names):
    """(tag, which are given): all, all but one in turn, none"""
    yield "all given", set(names)
    for name in names:
        yield "no " + name, set(names) - {name}
    yield "none given", set()


def single_queries(rec, rp, tag, k, vel):
    torch = rec.torch
    t = table(torch, SINGLE)
    six, ends = public(t, vel)
    d0, total = t[6].unsqueeze(1), (t[6] + t[7]).unsqueeze(1)
    lo, hi = windows(torch, k, t[6], 4, early=0.5)      # the zero width at 0.5, the inside window [0.75, 1.25] around the knots at 1
    tau = columns(torch, torch.tensor([[0.25, 0.75, 1.5, 2.5]] * N, dtype=torch.float64, device=DEV), k)
    level = columns(torch, torch.tensor([[0.5, 1.5, 5.0, 1.0]] * N, dtype=torch.float64, device=DEV), k)
    for order in (1, 2):
        rec.record("%s/eval order %d" % (tag, order), lambda *x: rp.trajectory_eval(*x[:7], vel0=x[7], vel2=x[8], order=order), six + [tau] + ends,
                   3, {6}, second=order == 2)
    out = rec.record(tag + "/crossing", lambda *x: (rp.trajectory_crossing(*x[:7], vel0=x[7], vel2=x[8]),), six + [level] + ends, 1, {6})
    if out is not None:
        rec.reached("crossing", out[0])
    for w_tag, given in subsets(("lo", "hi")):
        wl, wh = (lo if "lo" in given else None), (hi if "hi" in given else None)
        out = rec.record("%s/extrema/%s" % (tag, w_tag), lambda *x: rp.trajectory_extrema(*x[:8], vel0=x[8], vel2=x[9]), six + [wl, wh] + ends, 4,
                         {6, 7})
        if out is not None:
            time = torch.cat(out[4:], dim=1)
            missing = torch.isnan(torch.cat(out[:4], dim=1)) | torch.isnan(time)
            wide = lambda x: x.repeat(1, 4) if x is not None else None      # noqa: E731
            rec.sort("extrema", time, missing, (("LO", wide(wl)), ("HI", wide(wh)), ("END", total), ("KNOT", d0)))
        for order in (1, 2):
            out = rec.record("%s/integrals order %d/%s" % (tag, order, w_tag),
                             lambda *x: rp.trajectory_integrals(*x[:8], vel0=x[8], vel2=x[9], order=order), six + [wl, wh] + ends, 4, {6, 7},
                             second=order == 2)
            if out is not None:
                rec.count("integrals: values", ~torch.isnan(out[0]))
                rec.count("integrals: no value", torch.isnan(out[0]))
                rec.count("integrals: exactly 0", out[2] == 0)


def pair_inputs(torch, rows, vel):
    ta, tb = table(torch, [r[0] for r in rows]), table(torch, [r[1] for r in rows])
    a, a_ends = public(ta, vel)
    b, b_ends = public(tb, vel)
    delay = torch.tensor([r[2] for r in rows], dtype=torch.float64, device=DEV)
    return ta, tb, a, b, a_ends + b_ends, delay


def spline_of(six, ends):
    return list(six) + (list(ends) if any(e is not None for e in ends) else [])


def pair_queries(rec, rp, tag, k, vel):
    torch = rec.torch
    ta, tb, a, b, ends, delay = pair_inputs(torch, PAIRS, vel)
    lo, hi = windows(torch, k, ta[6], 0)
    delay = delay.unsqueeze(1).expand(N, k).contiguous()
    two = lambda x: (spline_of(x[:6], x[-4:-2]), spline_of(x[6:12], x[-2:]))      # noqa: E731
    col = lambda x: x.unsqueeze(1)      # noqa: E731
    whole = None
    for q_tag, given in subsets(("lo", "hi", "delay")):
        wl, wh, dl = (lo if "lo" in given else None), (hi if "hi" in given else None), (delay if "delay" in given else None)
        out = rec.record("%s/gap/%s" % (tag, q_tag), lambda *x: rp.trajectory_gap(*two(x), x[12], x[13], x[14]), a + b + [wl, wh, dl] + ends, 2,
                         {12, 13, 14})
        if out is not None:
            whole = out if whole is None else whole
            time = torch.cat(out[2:], dim=1)
            missing = torch.isnan(torch.cat(out[:2], dim=1)) | torch.isnan(time)
            wide = lambda x: x.repeat(1, 2) if x is not None else None      # noqa: E731
            shift = wide(dl) if dl is not None else torch.zeros_like(time)
            rec.sort("gap", time, missing, (("LO", wide(wl)), ("HI", wide(wh)), ("END_A", col(ta[6] + ta[7])), ("END_B", shift + col(tb[6] + tb[7])),
                                               ("KNOT_A", col(ta[6])), ("KNOT_B", shift + col(tb[6])), ("START", shift)), shift > 0)
        for order in (1, 2):
            out = rec.record("%s/tracking order %d/%s" % (tag, order, q_tag), lambda *x: rp.trajectory_tracking(*two(x), x[12], x[13], x[14], order=order),
                             a + b + [wl, wh, dl] + ends, 3, {12, 13, 14}, second=order == 2)
            if out is not None:
                rec.count("tracking: values", ~torch.isnan(out[0]))
                rec.count("tracking: no value", torch.isnan(out[0]))
    # a level between the extremes of the gap is met; the third query's is out of reach
    level = torch.ones((N, k), dtype=torch.float64, device=DEV)
    if whole is not None:
        level = torch.where(torch.isnan(whole[0]), level, 0.5 * (whole[0] + whole[1]))
    if k == 4:
        level[:, 2] = 1.0e6
    for q_tag, given in subsets(("level", "lo", "hi", "delay")):
        lv, wl, wh, dl = (level if "level" in given else None), (lo if "lo" in given else None), (hi if "hi" in given else None), \
            (delay if "delay" in given else None)
        out = rec.record("%s/meeting/%s" % (tag, q_tag), lambda *x: (rp.trajectory_meeting(*two(x), x[12], x[13], x[14], x[15]),),
                         a + b + [lv, wl, wh, dl] + ends, 1, {12, 13, 14, 15})
        if out is not None:
            rec.reached("meeting", out[0])


def vehicle_queries(rec, rp, tag, k, vel, d):
    torch = rec.torch
    ta, tb, a, b, ends, delay = pair_inputs(torch, VEHICLES, vel)
    scale = (1.0 + 0.25 * torch.arange(d, dtype=torch.float64, device=DEV)).unsqueeze(0)
    shift_c = (0.125 * torch.arange(d, dtype=torch.float64, device=DEV)).unsqueeze(0)

    def axes(x, j):      # (n,) -> (n, d): positions scaled and shifted, velocities scaled, durations repeated
        if x is None:
            return None
        x = x.unsqueeze(1)
        return (x * scale + shift_c if j < 3 else x * scale if j in (3, 6, 7) else x.expand(N, d)).contiguous()
    a = [axes(x, j) for j, x in enumerate(a)]
    b = [axes(x, j) for j, x in enumerate(b)]
    ends = [axes(x, 6) for x in ends]
    lo, hi = windows(torch, k, ta[6], 0)
    delay = delay.unsqueeze(1).expand(N, k).contiguous()
    two = lambda x: (spline_of(x[:6], x[-4:-2]), spline_of(x[6:12], x[-2:]))      # noqa: E731
    col = lambda x: x.unsqueeze(1)      # noqa: E731
    start = closest = None
    for q_tag, given in subsets(("lo", "hi", "delay")):
        wl, wh, dl = (lo if "lo" in given else None), (hi if "hi" in given else None), (delay if "delay" in given else None)
        out = rec.record("%s/separation/%s" % (tag, q_tag), lambda *x: rp.trajectory_separation(*two(x), x[12], x[13], x[14]),
                         a + b + [wl, wh, dl] + ends, 1, {12, 13, 14})
        if out is not None:
            value, time = out
            if closest is None:
                closest = value
                with torch.no_grad():
                    start = rp.trajectory_separation(*two(a + b + ends), lo, lo, delay)[0]
            missing = torch.isnan(value) | torch.isnan(time)
            shift = dl if dl is not None else torch.zeros_like(time)
            rec.sort("separation", time, missing, [("LO", wl), ("HI", wh)] + [("END of A", col(ta[6] + ta[7]))] * d
                        + [("END of B", shift + col(tb[6] + tb[7]))] * d + [("START", shift)], shift > 0)
    # a level half way between the squared distance at the window's start and the least one is reached; the third query's is not
    level = torch.ones((N, k), dtype=torch.float64, device=DEV)
    if closest is not None:
        level = torch.where(torch.isnan(start) | torch.isnan(closest), level, 0.5 * (start + closest))
    if k == 4:
        level[:, 2] = -1.0
    for q_tag, given in subsets(("lo", "hi", "delay")):
        wl, wh, dl = (lo if "lo" in given else None), (hi if "hi" in given else None), (delay if "delay" in given else None)
        out = rec.record("%s/contact/%s" % (tag, q_tag), lambda *x: (rp.trajectory_contact(*two(x), None, x[13], x[14], x[15], level_sq=x[12]),),
                         a + b + [level, wl, wh, dl] + ends, 1, {12, 13, 14, 15})
        if out is not None:
            rec.reached("contact", out[0])
    radius = torch.sqrt(level.clamp(min=0.0)) + 0.125
    rec.record(tag + "/contact/radius", lambda *x: (rp.trajectory_contact(*two(x), x[12], x[13], x[14], x[15]),), a + b + [radius, lo, hi, delay] + ends,
               1, {12, 13, 14, 15})


def compositions(rec, rp, tag, k, vel):
    """The min_time_* functions on generated problems, the queries placed by a solve beforehand"""
    torch = rec.torch
    gen = lambda seed, count: [torch.as_tensor(x).to(DEV) for x in rp.problems.generate(seed, 0, count, rp.problems.DIST_MONOTONE)]      # noqa: E731
    p, q = gen(11, N), gen(12, N)
    ends = [0.01 * (p[2] - p[0]), -0.01 * (p[2] - p[0])] if vel else [None, None]
    with torch.no_grad():
        solved = rp.min_time_solve(*p, vel0=ends[0], vel2=ends[1])
        total = (solved[1] + solved[2]).unsqueeze(1)
    frac = columns(torch, torch.tensor([[0.125, 0.25, 0.5, 0.625]] * N, dtype=torch.float64, device=DEV), k)
    lo, hi = frac * total, (frac + 0.25) * total
    level = p[0].unsqueeze(1) + frac * (p[2] - p[0]).unsqueeze(1)
    orders = (1,) if vel else (1, 2)      # with end velocities the solve is first order
    for order in orders:
        rec.record("%s/min_time_trajectory order %d" % (tag, order),
                   lambda *x: rp.min_time_trajectory(*x[:4], normalized=True, vel0=x[4], vel2=x[5], order=order)[:3], p + [frac] + ends, 3, {3},
                   second=order == 2)
        rec.record("%s/min_time_integrals order %d" % (tag, order), lambda *x: rp.min_time_integrals(*x[:5], vel0=x[5], vel2=x[6], order=order)[:4],
                   p + [lo, hi] + ends, 4, {3, 4}, second=order == 2)
    rec.record(tag + "/min_time_crossing", lambda *x: rp.min_time_crossing(*x[:4], vel0=x[4], vel2=x[5])[:1], p + [level] + ends, 1, {3})
    rec.record(tag + "/min_time_extrema", lambda *x: rp.min_time_extrema(*x[:5], vel0=x[5], vel2=x[6])[:8], p + [lo, hi] + ends, 4, {3, 4})
    if vel:
        return
    delay = 0.125 * total.expand(N, k).contiguous()
    gap = rec.record(tag + "/min_time_gap", lambda *x: rp.min_time_gap(x[:3], x[3:6], x[6], x[7], x[8])[:4], p + q + [lo, hi, delay], 2, {6, 7, 8})
    for order in (1, 2):
        rec.record("%s/min_time_tracking order %d" % (tag, order), lambda *x: rp.min_time_tracking(x[:3], x[3:6], x[6], x[7], x[8], order=order)[:3],
                   p + q + [lo, hi, delay], 3, {6, 7, 8}, second=order == 2)
    if gap is not None:
        meet = torch.where(torch.isnan(gap[0]), torch.ones_like(gap[0]), 0.5 * (gap[0] + gap[1]))
        rec.record(tag + "/min_time_meeting", lambda *x: rp.min_time_meeting(x[:3], x[3:6], x[6], x[7], x[8], x[9])[:1], p + q + [meet, lo, hi, delay],
                   1, {6, 7, 8, 9})
    for d in (1, 2, 3):
        pa = [x.reshape(N, d) for x in gen(13, N * d)]
        pb = [x.reshape(N, d) + 25.0 for x in gen(14, N * d)]
        sep = rec.record("%s/min_time_separation d %d" % (tag, d), lambda *x: rp.min_time_separation(x[:3], x[3:6], x[6], x[7], x[8])[:2],
                         pa + pb + [lo, hi, delay], 1, {6, 7, 8})
        if sep is not None:
            radius = torch.sqrt(torch.where(torch.isnan(sep[0]), torch.ones_like(sep[0]), sep[0]) * 1.5)
            rec.record("%s/min_time_contact d %d" % (tag, d), lambda *x: rp.min_time_contact(x[:3], x[3:6], x[6], x[7], x[8], x[9])[:1],
                       pa + pb + [radius, lo, hi, delay], 1, {6, 7, 8, 9})


def bits(path, tree):
    import numpy as np
    torch, rp = ab.load(tree)
    rec = Recorder(torch)
    for k in (1, 4):
        for vel in (True, False):
            tag = "k %d %s" % (k, "end velocities" if vel else "rest to rest")
            single_queries(rec, rp, tag, k, vel)
            pair_queries(rec, rp, tag, k, vel)
            for d in (1, 2, 3):
                vehicle_queries(rec, rp, "%s d %d" % (tag, d), k, vel, d)
            compositions(rec, rp, tag, k, vel)
            print("%s done: %d arrays so far" % (tag, len(rec.arrays)), flush=True)
    print("times by class:")
    for what, count in sorted(rec.classes.items()):
        print("    %-32s %d" % (what, count))
    empty = sorted(what for what, count in rec.classes.items() if count == 0)
    for what in empty:
        print("EMPTY CLASS: " + what)
    for text in rec.errors:
        print("RAISED: " + text)
    np.savez(path, **rec.arrays)
    print("%d arrays, %d bytes -> %s" % (len(rec.arrays), sum(x.nbytes for x in rec.arrays.values()), path))
    return 4 if rec.errors else 3 if empty else 0


def time_one(tree):
    import numpy as np
    torch, rp = ab.load(tree)
    k, d = 4, 3
    leaf = lambda x: x.detach().clone().requires_grad_(True) if x is not None else None      # noqa: E731
    t = table(torch, SINGLE)
    six, ends = public(t, True)
    lo, hi = windows(torch, k, t[6], 4, early=0.5)
    tau = torch.tensor([[0.25, 0.75, 1.5, 2.5]] * N, dtype=torch.float64, device=DEV)
    level = torch.tensor([[0.5, 1.5, 5.0, 1.0]] * N, dtype=torch.float64, device=DEV)
    six, ends, lo, hi, tau, level = [leaf(x) for x in six], [leaf(x) for x in ends], leaf(lo), leaf(hi), leaf(tau), leaf(level)
    _, _, a, b, pe, delay = pair_inputs(torch, PAIRS, True)
    pl, ph = windows(torch, k, a[4], 0)
    a, b, pe, pl, ph = [leaf(x) for x in a], [leaf(x) for x in b], [leaf(x) for x in pe], leaf(pl), leaf(ph)
    delay = leaf(delay.unsqueeze(1).expand(N, k).contiguous())
    sa, sb = a + pe[:2], b + pe[2:]
    _, _, va, vb, ve, _ = pair_inputs(torch, VEHICLES, True)
    wide = lambda x: leaf(x.unsqueeze(1).expand(N, d).contiguous())      # noqa: E731
    va, vb = [wide(x) for x in va + ve[:2]], [wide(x) for x in vb + ve[2:]]
    vb[0] = leaf(vb[0].detach() + torch.arange(d, dtype=torch.float64, device=DEV))      # (not on one line with A in every axis)
    meet = leaf(torch.full((N, k), -4.0, dtype=torch.float64, device=DEV))
    touch = leaf(torch.full((N, k), 16.0, dtype=torch.float64, device=DEV))
    kw = dict(vel0=ends[0], vel2=ends[1])
    functions = (
        ("trajectory_eval", lambda: rp.trajectory_eval(*six, tau, **kw)),
        ("trajectory_eval, order=2", lambda: rp.trajectory_eval(*six, tau, order=2, **kw)),
        ("trajectory_crossing", lambda: (rp.trajectory_crossing(*six, level, **kw),)),
        ("trajectory_extrema", lambda: rp.trajectory_extrema(*six, lo, hi, **kw)[:4]),
        ("trajectory_integrals", lambda: rp.trajectory_integrals(*six, lo, hi, **kw)),
        ("trajectory_integrals, order=2", lambda: rp.trajectory_integrals(*six, lo, hi, order=2, **kw)),
        ("trajectory_gap", lambda: rp.trajectory_gap(sa, sb, pl, ph, delay)[:2]),
        ("trajectory_meeting", lambda: (rp.trajectory_meeting(sa, sb, meet, pl, ph, delay),)),
        ("trajectory_tracking", lambda: rp.trajectory_tracking(sa, sb, pl, ph, delay)),
        ("trajectory_tracking, order=2", lambda: rp.trajectory_tracking(sa, sb, pl, ph, delay, order=2)),
        ("trajectory_separation", lambda: rp.trajectory_separation(va, vb, pl, ph, delay)[:1]),
        ("trajectory_contact", lambda: (rp.trajectory_contact(va, vb, None, pl, ph, delay, level_sq=touch),)),
    )
    leaves = six + ends + [lo, hi, tau, level] + sa + sb + [pl, ph, delay, meet, touch] + va + vb
    times = {name: [] for name, _ in functions}
    for r in range(ab.WARMUP + ab.REPS):
        for name, f in functions:
            torch.cuda.synchronize()
            t0 = clock.perf_counter()
            out = f()
            torch.autograd.grad(sum(torch.nan_to_num(o).sum() for o in out), leaves, allow_unused=True)
            torch.cuda.synchronize()
            if r >= ab.WARMUP:
                times[name].append(1e3 * (clock.perf_counter() - t0))
    print(json.dumps({name: float(np.median(x)) for name, x in times.items()}), flush=True)


if __name__ == "__main__":
    mode, rest = (sys.argv[1] if len(sys.argv) > 1 else ""), sys.argv[2:]
    if mode == "bits" and len(rest) in (1, 2):
        sys.exit(bits(rest[0], rest[1] if len(rest) == 2 else None))
    elif mode == "compare" and len(rest) == 2:
        sys.exit(ab.compare(*rest))
    elif mode == "time" and len(rest) in (1, 2):
        ab.__file__ = os.path.abspath(__file__)      # the timer starts `time-one` of the file its module names: this one's
        sys.exit(ab.timing(rest[0], rest[1] if len(rest) == 2 else None))
    elif mode == "time-one" and len(rest) in (0, 1):
        time_one(rest[0] if rest else None)
    else:
        sys.exit(__doc__)
