"""TEST INFRASTRUCTURE ONLY -- plain numpy restatement of the reference's chunks of a fixed number of bases and of
the squiggle trainer's batch of them, so that cases larger than the fixture have an expected answer.

Follows, line by line:
  taiyaki/signal_mapping.py:353-368  get_mapped_reference_region
  taiyaki/signal_mapping.py:459-477  get_current
  taiyaki/signal_mapping.py:479-513  _get_chunk (empty signal, max dwell)
  taiyaki/signal_mapping.py:556-594  get_chunk_with_sequence_length
  taiyaki/signal_mapping.py:680-716  Chunk.apply_filters
  taiyaki/chunk_selection.py:29-95   sample_chunks (accept loop, rejection counts)
  bin/train_squiggle.py:201-209      embed_sequence, concatenated currents, lengths
Pinned against tests/golden/chunks_seqlen.npz, which the genuine reference wrote
(tests/golden/make_golden_chunks_seqlen.py), by tests/test_chunks_seqlen_host.py.
"""
import numpy as np

REASONS = ("pass", "emptysequence", "emptysignal", "tooshort", "nullmapping", "pathbuffer", "meandwell", "maxdwell")
TINY = 0.00000001           # signal_mapping.py:607

# squiggle_match.pyx: the vertices of a tetrahedron, one per base (float32)
TETRAHEDRON = np.array([[1.0, 0.0, -1.0 / np.sqrt(2.0)], [-1.0, 0.0, -1.0 / np.sqrt(2.0)],
                        [0.0, 1.0, 1.0 / np.sqrt(2.0)], [0.0, -1.0, 1.0 / np.sqrt(2.0)]], dtype=np.float32)


def mapped_reference_region(read):
    """signal_mapping.py:353-368"""
    rts, siglen = np.asarray(read["Ref_to_signal"]), len(read["Dacs"])
    valid = np.where((rts >= 0) & (rts <= siglen))[0]
    if len(valid) == 0:
        return 0, 0
    return int(valid[0]), int(valid[-1])


def get_current(read, a, b, standardize=True):
    """signal_mapping.py:459-477: float64 arithmetic in this order"""
    cur = (read["Dacs"][a:b] + read["offset"]) * read["range"] / read["digitisation"]
    if standardize:
        cur = (cur - read["shift_frompA"]) / read["scale_frompA"]
    return cur


def chunk_with_sequence_length(read, chunk_bases, start_base, standardize=True):
    """signal_mapping.py:556-594 with an explicit start_base (bases into the mapped reference region).
    Returns dict(reason, current, sequence, max_dwell, start, refstart)."""
    lo, hi = mapped_reference_region(read)
    spare = (hi - lo) - chunk_bases
    if spare <= 0 or start_base >= spare:
        return dict(reason="tooshort")
    rts = read["Ref_to_signal"]
    r0 = start_base + lo
    r1 = r0 + chunk_bases
    a, b = int(rts[r0]), int(rts[r1])
    if r1 == r0:                                            # :498-499
        return dict(reason="emptysequence")
    if a == b:                                              # :500-501
        return dict(reason="emptysignal")
    dw = np.diff(rts[r0:r1])
    return dict(reason="pass", current=get_current(read, a, b, standardize), sequence=read["Reference"][r0:r1],
                max_dwell=int(dw.max()) if len(dw) else 1, start=a, refstart=r0)


def apply_filters(chunk, fp):
    """signal_mapping.py:680-716; fp = dict with the FILTER_PARAMETERS fields, None = not set."""
    if chunk["reason"] != "pass" or any(fp.get(k) is None for k in (
            "median_meandwell", "mad_meandwell", "model_stride", "path_buffer")):
        return chunk
    sig_len, seq_len = len(chunk["current"]), len(chunk["sequence"])
    if sig_len / (seq_len * fp["model_stride"]) <= fp["path_buffer"]:
        chunk["reason"] = "pathbuffer"
        return chunk
    mean_dwell = sig_len / (seq_len + TINY)
    if abs(mean_dwell - fp["median_meandwell"]) > fp["filter_mean_dwell"] * fp["mad_meandwell"]:
        chunk["reason"] = "meandwell"
        return chunk
    if chunk["max_dwell"] > fp["filter_max_dwell"] * fp["median_meandwell"]:
        chunk["reason"] = "maxdwell"
    return chunk


def sample_chunks(reads, nwant, chunk_bases, fp, candidates, standardize=True):
    """chunk_selection.py:29-95 with the random draws made explicit: candidates is a sequence of
    (read_number, start_base); at most int(nwant / filter_min_pass_fraction) are tried.
    Returns (accepted chunks, each with its read number, {reason: count}, attempts)."""
    limit = int(nwant / fp["filter_min_pass_fraction"])
    chunks, counts, attempts = [], {}, 0
    for rn, st in candidates:
        if len(chunks) >= nwant or attempts >= limit:
            break
        attempts += 1
        c = apply_filters(chunk_with_sequence_length(reads[rn], chunk_bases, st, standardize), fp)
        counts[c["reason"]] = counts.get(c["reason"], 0) + 1
        if c["reason"] == "pass":
            c["read"] = int(rn)
            chunks.append(c)
    return chunks, counts, attempts


def candidates_from_rng(reads, attempts, chunk_bases, rng):
    """The reference's draws made explicit: chunk_selection.py:78-80 `randint(nreads)`, then
    signal_mapping.py:584-586 `randint(spare_length)` only for reads with spare length."""
    out = []
    for _ in range(attempts):
        rn = int(rng.randint(len(reads)))
        lo, hi = mapped_reference_region(reads[rn])
        spare = (hi - lo) - chunk_bases
        out.append((rn, int(rng.randint(spare)) if spare > 0 else 0))
    return out


def med_mad(values):
    """maths.py med_mad with its default factor: (median, 1.4826 * median absolute deviation)"""
    values = np.asarray(values, dtype=np.float64)
    med = np.median(values)
    return float(med), float(1.4826 * np.median(np.abs(values - med)))


def mean_dwells(chunks):
    """Chunk.mean_dwell (signal_mapping.py:658-664) of accepted chunks"""
    return [len(c["current"]) / (len(c["sequence"]) + TINY) for c in chunks]


def assemble_batch(chunks, reverse=False):
    """bin/train_squiggle.py:201-209: seq_embed (bases, N, 3) float32, the flat current float32, the lengths,
    and the bases (bases, N) themselves."""
    if not chunks:          # (np.stack refuses an empty list; the reference's trainer would stop here)
        return np.zeros((0, 0, 3), np.float32), np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros((0, 0), np.int64)
    rev = (lambda x: np.flip(x)) if reverse else (lambda x: np.array(x))
    seqs = np.stack([rev(c["sequence"]).astype(np.int64) for c in chunks], axis=1)
    seq_embed = np.stack([TETRAHEDRON[rev(c["sequence"]).astype(np.int64)] for c in chunks], axis=1)
    signal = np.concatenate([rev(c["current"]) for c in chunks]).astype(np.float32)
    siglens = np.array([len(c["current"]) for c in chunks], dtype=np.int64)
    return seq_embed, signal, siglens, seqs


class ReplayRng:
    """Returns the draws the reference made (recorded by make_golden_chunks_seqlen.py), checking that each
    request has the bound the reference asked for; zeros once the record is exhausted (draws the reference never
    made: its loop had stopped)."""

    def __init__(self, draws):
        self.draws, self.k = np.asarray(draws), 0

    def randint(self, high):
        if self.k >= len(self.draws):
            return 0
        h, v = self.draws[self.k]
        assert h == high, (self.k, h, high)
        self.k += 1
        return int(v)


def filter_dict(spec, med=None, mad=None, on=True):
    return dict(filter_mean_dwell=spec["filter_mean_dwell"], filter_max_dwell=spec["filter_max_dwell"],
                filter_min_pass_fraction=spec["min_pass"], median_meandwell=med, mad_meandwell=mad,
                model_stride=spec["stride"] if on else None, path_buffer=spec["path_buffer"] if on else None)


# ---- what the tests compare with
def fields(golden, name, form):
    prefix = "%s/%s/" % (name, form)
    return {k[len(prefix):]: golden[k] for k in golden.files if k.startswith(prefix)}


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return (a.size == 0 and b.size == 0) or (a.shape == b.shape and np.array_equal(a, b))


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == b.dtype == np.float32
    return same(a.view(np.uint32), b.view(np.uint32))
