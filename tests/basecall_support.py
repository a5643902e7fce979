"""What tests/test_basecall_reads.py and tests/golden/make_golden_basecall_reads.py share: the seeded fixture signals,
the tail cases, and a numpy restatement of the basecaller's tail (stitch, collapse, quality characters)."""
import os
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "basecall_reads.npz")

STRIDE, CHUNK_BLOCKS, OVERLAP_BLOCKS = 5, 1000, 100
CHUNK, OVERLAP = CHUNK_BLOCKS * STRIDE, OVERLAP_BLOCKS * STRIDE         # samples

# name -> (length, seed, kind)
SIGNALS = {
    "len1": (1, 101, "plain"),
    "len2": (2, 102, "plain"),
    "len4999": (4999, 103, "plain"),            # shorter than one chunk
    "len5000": (5000, 104, "plain"),            # exactly one chunk
    "len5001": (5001, 105, "plain"),
    "len9500": (9500, 106, "plain"),
    "len23456": (23456, 107, "plain"),
    "len100003": (100003, 108, "plain"),
    "ties_even": (30000, 109, "ties"),          # about 200 distinct values
    "ties_odd": (30001, 110, "ties"),
    "constant": (7000, 111, "constant"),
}


def signal(name):
    """A seeded float32 signal in picoampere-like units (a slow drift under the noise, so chunks differ)."""
    n, seed, kind = SIGNALS[name]
    rs = np.random.RandomState(seed)
    if kind == "constant":
        return np.full(n, 85.25, dtype=np.float32)
    x = 90.0 + 12.0 * rs.standard_normal(n) + 3.0 * np.sin(np.arange(n) / 700.0)
    if kind == "ties":
        x = np.round(x * 2.5) / 2.5
    return x.astype(np.float32)


# tail cases: name -> blocks per chunk, stride, overlap (samples), chunks, seed, samples cut off the last chunk
TAILS = {
    "one": dict(T=300, stride=5, overlap=100, N=1, seed=71, ragged=0),
    "two": dict(T=300, stride=5, overlap=100, N=2, seed=72, ragged=437),
    "twenty": dict(T=300, stride=5, overlap=100, N=20, seed=73, ragged=123),
    "stride2": dict(T=250, stride=2, overlap=40, N=7, seed=74, ragged=11),
}
QSETTINGS = {"q10": (1.0, 0.0), "q0903": (0.9, 0.3)}


def tail_siglen(spec):
    chunk = spec["T"] * spec["stride"]
    return chunk + (spec["N"] - 1) * (chunk - spec["overlap"]) - spec["ragged"]


def tail_scores(spec):
    """Confident scores with realistic dwell (runs of equal states): one random alignment per chunk.  Confidence is
    held to on = 2 / off = -1: every error probability then lies well inside (1e-9, 1), where the reference's
    quality arithmetic is defined (at on = 3 / off = -2 some are exactly 0)."""
    from taiyaki_amd import synth
    seqlens = (spec["T"] * (0.35 + 0.2 * np.random.RandomState(spec["seed"]).uniform(size=spec["N"]))).astype(np.int32)
    inp = synth.crf_case(spec["T"], spec["N"], spec["seed"], seqlens=seqlens)
    return synth.confident_scores(inp, spec["seed"] + 1000, on=2.0, off=-1.0)["scores"]


def crc(a):
    return zlib.crc32(np.ascontiguousarray(a).tobytes())


def load():
    return np.load(GOLDEN)


# ----------------------------------------------------------------------------------------------------------------------
# the tail, restated in numpy (numpy doing numpy's arithmetic: exact against the reference's strings)
# ----------------------------------------------------------------------------------------------------------------------
def cuts(starts, ends, stride, nrow):
    """Rows [lo, hi) that stitch_chunks(path_stitching=False) keeps of every chunk (basecall_helpers.py:64-94)."""
    n = len(starts)
    if n == 1:
        return [(0, nrow)]
    out = []
    for i in range(n):
        if i == 0:
            lo, hi = starts[0] // stride, (ends[0] + starts[1]) // (2 * stride)
        elif i < n - 1:
            lo = (ends[i - 1] - starts[i]) // (2 * stride)
            hi = (ends[i] + starts[i + 1] - 2 * starts[i]) // (2 * stride)
        else:
            lo, hi = (ends[-2] - starts[-1]) // (2 * stride), (ends[-1] - starts[-1]) // stride
        out.append((int(min(lo, nrow)), int(min(hi, nrow))))
    return out


def tail(path, errprobs, starts, ends, stride, alphabet="ACGT", qscore_scale=1.0, qscore_offset=0.0):
    """(sequence, quality string or None, stitched path) of one read's per-chunk paths (nblk + 1, nchunks)."""
    nrow = path.shape[0]
    keep = cuts(starts, ends, stride, nrow)
    sp = np.concatenate([path[lo:hi, i] for i, (lo, hi) in enumerate(keep)])
    move = np.zeros(len(sp), dtype=bool)
    move[1:] = sp[1:] != sp[:-1]
    letters = np.frombuffer(alphabet.encode(), dtype="u1")
    seq = letters[sp[move] % len(alphabet)].tobytes().decode()
    if errprobs is None:
        return seq, None, sp
    se = np.concatenate([errprobs[lo:hi, i] for i, (lo, hi) in enumerate(keep)]).astype(np.float32)
    q = qscore_scale * (-10.0 * np.log10(se[move])) + qscore_offset         # qscores.py:30-55, float32 throughout
    return seq, (q + 33 + 0.5).astype(np.int8).tobytes().decode("ascii"), sp


def qstrings_close(got, want):
    """The rule this project uses for device-computed quality characters (tests/test_basecall_consumers.py:89-92):
    equal length, no character more than one step off, fewer than 1 % of them different."""
    if len(got) != len(want):
        return False
    diff = np.abs(np.frombuffer(got.encode(), np.uint8).astype(int) - np.frombuffer(want.encode(), np.uint8))
    return bool(diff.max(initial=0) <= 1 and (diff > 0).mean() < 0.01) if len(want) else True
