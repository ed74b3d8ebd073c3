"""The inputs of tests/shortlist_gpu_cases.py and the conditions they are held to, in numpy alone, so that tests/test_shortlist_cpu.py can
check the conditions without a device ("The shortlist under chosen flags"): which problems the sieve keeps, chosen
flag by flag; the standing scenes and the per-pair levels that make the sieve keep exactly those; and how k_shortlist_scan's one block
shares the chunks of a size among its threads."""
import numpy as np

CHUNK = 2048             # trajectory.hip's kShortChunk: flags per chunk, 256 threads x 8 flags
SCAN_THREADS = 256       # kShortBlock: the threads of k_shortlist_scan's one block
APART = 10.0             # the distance between neighbouring standing vehicles of three; two stand 20 apart
CULLED, CONTACT = 1.0, 400.0      # levels (squared distances): provably out of reach at 10 and at 20 apart; where a pair 20 apart is
# problems: around one thread's eight flags, around one chunk, two chunks and a ragged third; 256 chunks (each = 1, every scan thread
# busy); 257 (each = 2, the last chunk one flag, threads above 128 idle); 385 (thread 192 has one chunk); 518 (each = 3, thread 172 has two)
SIZES = (1, 7, 8, 9, 2047, 2048, 2049, 4101, 524288, 524289, 786437, 1060000)
LARGEST = (786437, 1060000)
PATTERNS = ("nothing", "everything", "the first problem", "the last problem", "the first flag of every chunk", "the last flag of every chunk",
            "every eighth", "one whole chunk", "all but one whole chunk", "random 1/1000", "random 1/2", "random 999/1000")
AT_THE_LARGEST = ("the last problem", "the last flag of every chunk", "random 1/2")
DENSITY = {"random 1/1000": 0.001, "random 1/2": 0.5, "random 999/1000": 0.999}
SECOND_TRIP_N, SECOND_TRIP_EVERY = 300001, 64      # every 64th problem culled: 295,313 listed, more than 2,048 trips of 128


def chunks_of(n):
    return (n + CHUNK - 1) // CHUNK


def scan_share(n):
    """(chunks, each, the number of chunks of each of k_shortlist_scan's 256 threads): thread t takes [t each, (t + 1) each) of the chunks"""
    chunks = chunks_of(n)
    each = (chunks + SCAN_THREADS - 1) // SCAN_THREADS
    t = np.arange(SCAN_THREADS)
    return chunks, each, np.clip(chunks - t * each, 0, each)


def middle_chunk(n):
    """(first, end) of the whole chunk of 'one whole chunk': the middle one, the lower of two -- never the ragged last one of several"""
    c = (chunks_of(n) - 1) // 2
    return c * CHUNK, min((c + 1) * CHUNK, n)


def pattern(name, n):
    """(n,) bool: the problems the sieve is to keep"""
    p = np.arange(n)
    if name in DENSITY:
        return np.random.default_rng(3000 + PATTERNS.index(name)).uniform(size=n) < DENSITY[name]
    if name in ("one whole chunk", "all but one whole chunk"):
        first, end = middle_chunk(n)
        inside = (p >= first) & (p < end)
        return inside if name == "one whole chunk" else ~inside
    return {"nothing": p < 0, "everything": p >= 0, "the first problem": p == 0, "the last problem": p == n - 1,
            "the first flag of every chunk": p % CHUNK == 0, "the last flag of every chunk": (p % CHUNK == CHUNK - 1) | (p == n - 1),
            "every eighth": p % 8 == 7}[name]


def levels_of(keep):
    """The per-pair levels that make the sieve keep exactly `keep` (any shape): CULLED where not; where kept CONTACT, and NaN -- kept, and
    the search returns NaN -- for every third of the kept"""
    keep = np.asarray(keep, dtype=bool)
    rank = np.cumsum(keep.reshape(-1)).reshape(keep.shape)
    return np.where(keep, np.where(rank % 3 == 0, np.nan, CONTACT), CULLED)


def places(m):
    """Where the m standing vehicles are: 0, 10 and 20; two vehicles at 0 and 20, so that their one pair is at the level CONTACT"""
    assert m in (2, 3)
    return APART * (np.arange(3, dtype=np.float64) if m == 3 else np.array([0.0, 2.0]))


def standing_fleet(n, m):
    """One axis, eight (n, m) arrays in the table's order: vehicle v stands at places(m)[v] for 1 + 1"""
    at = np.ascontiguousarray(np.broadcast_to(places(m), (n, m)))
    zero, one = np.zeros((n, m)), np.ones((n, m))
    return [[at, at.copy(), at.copy(), zero, zero.copy(), zero.copy(), one, one.copy()]]


def windows(n, k, seed=3100):
    """(lo, hi), (n, k): a start of U(0, 1) rounded to 2^-20, inside every vehicle's 1 + 1, and the end 0.5 later -- a problem's time is its own start"""
    lo = np.round(np.random.default_rng(seed).uniform(0.0, 1.0, (n, k)) * 2.0 ** 20) / 2.0 ** 20
    return np.ascontiguousarray(lo), np.ascontiguousarray(lo + 0.5)


def expected_times(level, lo, m):
    """The plain expectation: the window's start where the level is CONTACT and the pair is at it -- the entry returns the earliest time at
    which the squared distance is at the level, and a standing pair's is at its own only: 20 apart --, NaN elsewhere.  level
    (n, pairs, k), lo (n, k)."""
    first, second = np.triu_indices(m, 1)
    at_it = ((places(m)[second] - places(m)[first]) ** 2 == CONTACT)[None, :, None]
    return np.where((level == CONTACT) & at_it, np.broadcast_to(lo[:, None, :], level.shape), np.nan)


def second_trip_keep():
    p = np.arange(SECOND_TRIP_N)
    return p % SECOND_TRIP_EVERY != 0


def approaching_fleet(n, seed=3200):
    """m = 2, one axis: vehicle 0 stands at 0; vehicle 1 runs from APART towards it at the constant velocity v ~ U(1, 2) of its scene, for
    1 + 1.  Over a window [0, 0.5] the boxes stay at least APART - 1 = 9 apart; the distance r is reached at (APART - r) / v."""
    v = np.random.default_rng(seed).uniform(1.0, 2.0, n)
    zero, one = np.zeros(n), np.ones(n)
    first = [zero, zero, zero, zero, zero, zero, one, one]
    second = [APART + zero, APART - v, APART - 2 * v, -v, -v, -v, one, one]
    return [[np.ascontiguousarray(np.stack([a, b], axis=1)) for a, b in zip(first, second)]], v


def approaching_levels(keep, seed=3201):
    """(n, 1, 1): CULLED where not kept; where kept r^2 with r ~ U(9.6, 9.9): more than the boxes' gap, which is APART - v / 2 <= 9.5, and reached inside [0, 0.5]"""
    r = np.random.default_rng(seed).uniform(9.6, 9.9, keep.shape)
    return np.ascontiguousarray(np.where(keep, r * r, CULLED)[:, None, None])
