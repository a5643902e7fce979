"""What tests/test_basecall_mods.py and tests/golden/make_golden_mod_weights.py share: the seeded golden cases, a numpy
restatement of the stitched contract of tk_basecall_mod_weights_dev (include/taiyaki_amd_basecall.h, (f)) and the
comparison of modified-base score arrays, which is one of bit patterns: the kernel only copies."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "mod_weights_small.npz")

CAN_NMODS = ((1, 1, 0, 0), (2, 0, 1, 0), (0, 0, 0, 1))
BATCH_T = 40            # the cases of one can_nmods at this T form a batch: random, no move at all, a move at every block
KINDS = ("random", "nomove", "allmove")


def golden_cases():
    """[(name, can_nmods, T, kind, seed)]"""
    out = []
    for ci, cm in enumerate(CAN_NMODS):
        for ki, kind in enumerate(KINDS):
            out.append(("m%d/T%d/%s" % (ci, BATCH_T, kind), cm, BATCH_T, kind, 100 * ci + ki))
        for ti, T in enumerate((1, 2, 7, 60)):
            out.append(("m%d/T%d/random" % (ci, T), cm, T, "random", 100 * ci + 10 + ti))
    return out


def flipflop_path(nrow, seed, kind="random", nbase=4, stay=0.6):
    """A flip-flop-legal state path of `nrow` rows: a random base sequence, flip-flop coded (a repeated base alternates
    between its flip and its flop state), every state held for a geometric number of rows (`stay`)."""
    from taiyaki_amd import synth
    rs = np.random.RandomState(seed)
    if kind == "nomove":
        return np.full(nrow, int(rs.randint(2 * nbase)), dtype=np.int64)
    moves = np.ones(nrow, dtype=bool) if kind == "allmove" else rs.uniform(size=nrow) >= stay
    moves[0] = False
    codes = synth.flipflop_code(rs.randint(nbase, size=int(moves.sum()) + 1), nbase)
    return codes[np.cumsum(moves)].astype(np.int64)


def weights(shape, seed):
    """float32 log-probability-like values, all different, with the patterns a copy must not disturb among them."""
    rs = np.random.RandomState(seed)
    w = (-np.abs(rs.standard_normal(shape)) - rs.uniform(size=shape) * 1e-3).astype(np.float32)
    flat = w.reshape(-1)
    for i, v in enumerate((np.float32(-0.0), np.float32(-1e-42), np.float32(-np.inf), np.float32(-3.4e38))):
        if flat.size > 4 * (i + 1):
            flat[rs.randint(flat.size)] = v
    return w


def golden_inputs(can_nmods, T, kind, seed):
    return weights((T, len(can_nmods) + sum(can_nmods)), seed + 5000), flipflop_path(T + 1, seed, kind, len(can_nmods))


# ----------------------------------------------------------------------------------------------------------------------
# the contract, restated
# ----------------------------------------------------------------------------------------------------------------------
def column_map(can_nmods):
    """[(canonical base, column of a weight row)] of every output column: the m-th modification of base b sits at
    off_b + 1 + m, off_b = sum over b' < b of (can_nmods[b'] + 1)."""
    out, off = [], 0
    for b, n in enumerate(can_nmods):
        out += [(b, off + 1 + m) for m in range(n)]
        off += 1 + n
    return out


def moves_to_mods(W, P, can_nmods):
    """W (>= len(P) - 1, ncat) float32 weight rows, P the state of every row -> (moves, nmod) float32: row k >= 1 is a
    move when P[k] != P[k - 1]; the i-th move, into base P[k] % nbase, takes its base's modifications from W[k - 1];
    every other column is NaN."""
    P, cols = np.asarray(P), column_map(can_nmods)
    k = np.flatnonzero(P[1:] != P[:-1]) + 1
    out = np.full((len(k), len(cols)), np.nan, dtype=np.float32)
    base = P[k] % len(can_nmods)
    assert len(k) == 0 or k.max() - 1 < len(W)
    for j, (b, src) in enumerate(cols):
        out[base == b, j] = W[k[base == b] - 1, src]
    return out


def stitched_mods(path, mod_weights, starts, ends, stride, can_nmods):
    """One read: its per-chunk paths (nblk + 1, nchunks) and weights (nblk, nchunks, ncat) -> (seqlen, nmod): both
    stitched by basecall_helpers.stitch_chunks (path_stitching=False, the same cuts), then the move rule."""
    import torch
    from taiyaki_amd import basecall_helpers
    P = basecall_helpers.stitch_chunks(torch.from_numpy(np.ascontiguousarray(path)), starts, ends, stride).numpy()
    W = basecall_helpers.stitch_chunks(torch.from_numpy(np.ascontiguousarray(mod_weights)), starts, ends, stride).numpy()
    return moves_to_mods(W[:len(P) - 1], P, can_nmods)


def same_bits(got, want):
    """Equal shapes, equal NaN masks, and equal float32 bit patterns wherever there is no NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != np.float32 or want.dtype != np.float32 or got.shape != want.shape:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(np.ascontiguousarray(got).view(np.uint32)[~nan],
                               np.ascontiguousarray(want).view(np.uint32)[~nan]))
