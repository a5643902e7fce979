"""The alignment of include/taiyaki_amd_align.h stated on the host, for tests/test_align_host.py and tests/test_align.py.

`align_plain` is the recurrence as written: pairs of ints, the full table, Python's tuple order as the lexicographic
minimum.  `align_banded` is the same over the band of `band_rule` only.  `align_rows` gives `align_plain`'s answer a row
at a time in numpy (for the sizes the device tests use); test_align_host.py holds it against `align_plain`."""
import numpy as np

BIG = 1 << 32           # `align_rows`: a cell is D * BIG - M in int64


def codes(seq):
    """str | bytes | array of small ints -> uint8 array"""
    if isinstance(seq, str):
        seq = seq.encode()
    if isinstance(seq, (bytes, bytearray)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    return np.asarray(seq, dtype=np.uint8)


def band_rule(m, n, t):
    """Section "Band" of the definition: the diagonals j - i swept for max_distance t (None: all), as (first, last) clipped
    to the diagonals that cross the (m + 1) x (n + 1) table; None where t < |n - m|."""
    if t is None:
        return -m, n
    if t < abs(n - m):
        return None
    p = (t - abs(n - m)) // 2
    lo, hi = (-p, (n - m) + p) if n >= m else ((n - m) - p, p)
    return max(lo, -m), min(hi, n)


def cells_per_lane(width):
    """the sweep that takes a band of `width` diagonals: 1, 2, 4, 8, 16 cells per lane in registers, odd counts in LDS"""
    c = -(-width // 64)
    for reg in (1, 2, 4, 8, 16):
        if c <= reg:
            return reg
    return c | 1


def _sweep(q, r, inside):
    m, n = len(q), len(r)
    none = (1 << 60, 0)
    cell = {}
    for i in range(m + 1):
        for j in range(n + 1):
            if not inside(i, j):
                continue
            if i == 0 or j == 0:
                cell[i, j] = (i + j, 0)
                continue
            d, mt = cell.get((i - 1, j - 1), none)
            best = (d, mt - 1) if q[i - 1] == r[j - 1] else (d + 1, mt)
            for d, mt in (cell.get((i - 1, j), none), cell.get((i, j - 1), none)):
                best = min(best, (d + 1, mt))
            cell[i, j] = best
    d, negm = cell[m, n]
    return d, -negm


def align_plain(q, r):
    """(D, M) of the full table"""
    return _sweep(list(codes(q)), list(codes(r)), lambda i, j: True)


def align_banded(q, r, t):
    """(D, M, exact) as the entry points report them for max_distance t (None: every diagonal)"""
    q, r = list(codes(q)), list(codes(r))
    band = band_rule(len(q), len(r), t)
    if band is None:
        return max(len(q), len(r)), 0, 0
    d, mt = _sweep(q, r, lambda i, j: band[0] <= j - i <= band[1])
    return d, mt, int(t is None or d <= t)


def align_rows(q, r):
    """(D, M) of the full table, a row per numpy step: the left neighbour is a prefix minimum of cell - j * BIG"""
    q, r = codes(q), codes(r)
    n = len(r)
    ramp = np.arange(n + 1, dtype=np.int64) * BIG
    row = ramp.copy()
    for i in range(1, len(q) + 1):
        new = np.empty_like(row)
        new[0] = i * BIG
        new[1:] = np.minimum(row[:-1] + np.where(r == q[i - 1], -1, BIG), row[1:] + BIG)
        row = np.minimum.accumulate(new - ramp) + ramp
    key = int(row[n])
    d = -(-key // BIG)
    return d, d * BIG - key


def mutate(seq, rate, rng, nbase=4):
    """substitutions, insertions and deletions, `rate` of the positions in all"""
    out = []
    for c in codes(seq):
        u = rng.random_sample()
        if u < rate / 3:
            out.append((int(c) + 1 + rng.randint(nbase - 1)) % nbase)
        elif u < 2 * rate / 3:
            out.extend([int(c), rng.randint(nbase)])
        elif u >= rate:
            out.append(int(c))
    return np.array(out, dtype=np.uint8)


def collapse(path, nbase):
    """flipflopfings.path_to_str on codes: state % nbase where the state differs from its predecessor, first included"""
    path = np.asarray(path)
    move = np.ediff1d(path, to_begin=1) != 0
    return (path[move] % nbase).astype(np.uint8)
