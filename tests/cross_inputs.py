"""The inputs of tests/cross_gpu_cases.py and the conditions they are held to, in numpy alone, so that the conditions can be measured
without a device: two fleets out of fleet_gpu_cases.fleet_inputs' generator, the windows over a scene's common
domain, the pair entry's view of the m_a m_b pairs, the levels in both layouts, and the shares the section quotes
(`python tests/cross_inputs.py` prints them)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import contact_ref as cf  # noqa: E402
import separation_ref as sr  # noqa: E402
import trajectory_ref as tr  # noqa: E402

# (m_a, m_b, n), the ks and the ds: with 128 problems per trip, 3 x 5 x 20 is 300 problems -- three trips, the last partial, 15-pair scenes
# straddling the trip ends; 1 x 43 x 3 and 43 x 1 x 3 are 129 -- a trailing single problem, with k = 7 a single trailing query, and a fleet
# of one on either side; 1 x 1 x 300 is the pair call itself; 7 x 300 x 1 one scene of 2,100 pairs, m_b beyond the fleet entries' 256
SHAPES = {"3x5x20": (3, 5, 20, (1, 7, 8), (1, 2, 3)), "1x43x3": (1, 43, 3, (1, 7, 8), (1, 2, 3)), "43x1x3": (43, 1, 3, (1, 7, 8), (1, 2, 3)),
          "1x1x300": (1, 1, 300, (1, 7, 8), (1, 2, 3)), "7x300x1": (7, 300, 1, (1,), (2,))}
# (shape, d, k) -> the seed of contact_ref.levels where 300 + d misses a condition, 25 % of the times finite and 10 % NaN in both layouts
# (section 34): three scenes have 3 k per-scene levels, each for 43 pairs, so the per-scene shares move in large steps from seed to seed.
# The first seed 300 + d + 10 t, t = 1, 2, ..., that clears both conditions by two points on the CPU (contact_f64)
LEVEL_SEEDS = {("1x43x3", 1, 1): 311, ("1x43x3", 2, 1): 312, ("1x43x3", 2, 8): 312, ("1x43x3", 3, 7): 313, ("1x43x3", 3, 8): 1113,
               ("43x1x3", 3, 7): 343, ("43x1x3", 3, 8): 743}


def level_seed(shape, d, k):
    return LEVEL_SEEDS.get((shape, d, k), 300 + d)


def fleets(n, m_a, m_b, d):
    """(A, B), each d lists (the axes) of eight (n, m) arrays in the table's order: vehicle v of the m_a + m_b, axis c, is
    random_states(n, 1 + c + 3 v); A holds the first m_a -- fleet_gpu_cases.fleet_inputs(n, m_a, d) -- and B the m_b after them."""
    per = [[tr.random_states(n, 1 + c + 3 * v) for v in range(m_a + m_b)] for c in range(d)]
    take = lambda first, count: [[np.ascontiguousarray(np.stack([per[c][v][f] for v in range(first, first + count)], axis=1))      # noqa: E731
                                  for f in range(8)] for c in range(d)]
    return take(0, m_a), take(m_a, m_b)


def scene_windows(fleet_a, fleet_b, k, seed):
    """Section 18's windows over each scene's domain, [0, the smallest total time of its (m_a + m_b) d splines]: (lo, hi), (n, k)."""
    n = fleet_a[0][0].shape[0]
    every = [[axis[f][:, v] for f in range(8)] for fleet in (fleet_a, fleet_b) for axis in fleet for v in range(axis[0].shape[1])]
    return sr.windows(every, every, np.zeros((n, k)), seed)


def pairs_of(m_a, m_b):
    r = np.arange(m_a * m_b)
    return r // m_b, r % m_b


def gathered(fleet_a, fleet_b, lo, hi):
    """The pair entry's inputs: vehicles A and B as lists of d splines of n pairs values, problem s pairs + r, and the windows repeated."""
    i, j = pairs_of(fleet_a[0][0].shape[1], fleet_b[0][0].shape[1])
    a = [[np.ascontiguousarray(x[:, i].reshape(-1)) for x in axis] for axis in fleet_a]
    b = [[np.ascontiguousarray(x[:, j].reshape(-1)) for x in axis] for axis in fleet_b]
    rep = lambda w: np.ascontiguousarray(np.repeat(w, len(i), axis=0)) if w is not None else None      # noqa: E731
    return a, b, rep(lo), rep(hi)


def scene_levels(per_pair):
    """the per-scene level of scene s and query q: the per-pair level of pair (s + q) mod pairs"""
    n, pairs, k = per_pair.shape
    pick = (np.arange(n)[:, None] + np.arange(k)[None, :]) % pairs
    return np.ascontiguousarray(np.take_along_axis(per_pair, pick[:, None, :], axis=1)[:, 0, :])


def levels_of(fleet_a, fleet_b, lo, hi, seed):
    """(the per-pair levels (n, pairs, k), the per-scene levels (n, k)): contact_ref.levels on the gathered pairs"""
    n = fleet_a[0][0].shape[0]
    a, b, rl, rh = gathered(fleet_a, fleet_b, lo, hi)
    per_pair = np.ascontiguousarray(cf.levels(a, b, rl, rh, np.zeros(rl.shape), seed)[0].reshape(n, -1, rl.shape[1]))
    return per_pair, scene_levels(per_pair)


def wide_level(level, pairs):
    """a level, per pair or per scene, as the pair entry's (n pairs, k)"""
    return np.ascontiguousarray(level.reshape(-1, level.shape[-1]) if level.ndim == 3 else np.repeat(level, pairs, axis=0))


def shares(fleet_a, fleet_b, level, lo, hi):
    """(the share of the times that are finite, the share that are NaN) by contact_ref.contact_f64 on the gathered pairs"""
    a, b, rl, rh = gathered(fleet_a, fleet_b, lo, hi)
    pairs = len(a[0][0]) // fleet_a[0][0].shape[0]
    time = cf.contact_f64(a, b, wide_level(level, pairs), rl, rh, np.zeros(rl.shape))[0]
    return float(np.isfinite(time).mean()), float(np.isnan(time).mean())


def main():
    worst = {}
    for shape, (m_a, m_b, n, ks, ds) in SHAPES.items():
        for d in ds:
            fleet_a, fleet_b = fleets(n, m_a, m_b, d)
            for k in ks:
                lo, hi = scene_windows(fleet_a, fleet_b, k, 900 + k)
                for layout, level in zip(("per pair", "per scene"), levels_of(fleet_a, fleet_b, lo, hi, level_seed(shape, d, k))):
                    finite, missing = shares(fleet_a, fleet_b, level, lo, hi)
                    print("%s d = %d k = %d, level %s: %.1f %% finite, %.1f %% NaN%s"
                          % (shape, d, k, layout, 100 * finite, 100 * missing, "" if finite >= 0.25 and missing >= 0.10 else "   <-- misses a condition"))
                    w = worst.setdefault(layout, [1.0, 1.0])
                    w[0], w[1] = min(w[0], finite), min(w[1], missing)
    for layout, (finite, missing) in worst.items():
        print("level %s: at least %.1f %% finite and %.1f %% NaN on every shape" % (layout, 100 * finite, 100 * missing))


if __name__ == "__main__":
    main()
