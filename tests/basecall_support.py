"""What tests/test_basecall_reads.py and tests/golden/make_golden_basecall_reads.py share: the seeded fixture signals,
the tail cases, and a numpy restatement of the basecaller's tail (stitch, collapse, quality characters).

For tests/test_basecall_glue_edges.py as well: the launches of the glue kernels at the C ABI (every output between
sentinels), the stand-in network `columnwise`, and the seeded generators of that file's inputs -- signals for every branch
of the radix selection, read lengths for the chunk plan past 256 reads, read geometries and paths for the shared walk."""
import ctypes
import functools
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


# ----------------------------------------------------------------------------------------------------------------------
# the glue kernels at the C ABI (GPU tests).  Every kernel is launched once per call; outputs lie between sentinels.
# ----------------------------------------------------------------------------------------------------------------------
BAD_SIGNAL, CHUNK_PLAN = 128, 256           # TK_STATUS_BAD_SIGNAL, TK_STATUS_CHUNK_PLAN
GUARD = 64                                  # elements of sentinel in front of and behind a guarded buffer


def dev_ptr(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def ok(rc):
    assert rc == 0, rc


def _dev(a, dtype, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).astype(dtype)).to(dev)


def upload(signals, dev):
    """The reads laid back to back -> (flat signal, sig_off, lengths); one float nobody owns where there is no sample."""
    lens = np.array([len(s) for s in signals], dtype=np.int64)
    flat = np.concatenate(list(signals) + ([np.zeros(1)] if lens.sum() == 0 else []))
    return _dev(flat, np.float32, dev), _dev(np.concatenate([[0], np.cumsum(lens)]), np.int64, dev), lens


def med_mad_dev(signals, dev):
    """tk_signal_med_mad_dev on all the signals in one launch -> (med, mad, status)"""
    import torch
    from taiyaki_amd import _lib
    flat, off, _ = upload(signals, dev)
    med = torch.empty(len(signals), dtype=torch.float32, device=dev)
    mad, status = torch.empty_like(med), torch.zeros(1, dtype=torch.int32, device=dev)
    ok(_lib.basecall_lib().tk_signal_med_mad_dev(dev_ptr(flat), dev_ptr(off), len(signals), dev_ptr(med), dev_ptr(mad),
                                                 dev_ptr(status), None))
    return med.cpu().numpy(), mad.cpu().numpy(), int(status.item())


def _guarded(n, dtype, fill, dev):
    """(the whole buffer, its n elements between two guards of GUARD elements): all of it holds `fill`"""
    import torch
    whole = torch.full((n + 2 * GUARD,), fill, dtype=dtype, device=dev)
    return whole, whole[GUARD:GUARD + n]


def _guards_hold(whole, fill):
    w = whole.cpu().numpy()
    return bool((w[:GUARD] == fill).all() and (w[len(w) - GUARD:] == fill).all())


def gather_dev(signals, shift, scale, dev, chunk=CHUNK, overlap=OVERLAP, total=None):
    """tk_basecall_gather_chunks_dev -> (chunks (chunk, total, 1), starts, ends, read_chunk_off, status).  `total`: the
    chunk count handed to the kernel, by default what the lengths give.  Every buffer the kernels write is allocated
    for exactly `total` chunks between sentinels, and nothing may have been written outside it."""
    import torch
    from taiyaki_amd import _lib, basecall
    L = _lib.basecall_lib()
    flat, off, lens = upload(signals, dev)
    if total is None:
        total = int(basecall.chunk_counts(lens, chunk, overlap).sum())
    ws_bytes = L.tk_basecall_gather_workspace_bytes(total)
    assert ws_bytes % 16 == 0 and ws_bytes >= 4 * total
    bufs = dict(chunks=_guarded(chunk * total, torch.float32, 777.0, dev), starts=_guarded(total, torch.int64, -7, dev),
                ends=_guarded(total, torch.int64, -7, dev), rco=_guarded(len(signals) + 1, torch.int64, -7, dev),
                ws=_guarded(ws_bytes // 4, torch.int32, -7, dev))
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    sh, sc = (_dev(np.asarray(v, dtype=np.float32), np.float32, dev) for v in (shift, scale))
    ptr = {k: dev_ptr(v[1]) for k, v in bufs.items()}
    assert ptr["ws"].value % 16 == 0
    ok(L.tk_basecall_gather_chunks_dev(dev_ptr(flat), dev_ptr(off), len(signals), int(lens.sum()), dev_ptr(sh), dev_ptr(sc),
                                       chunk, overlap, total, ptr["chunks"], ptr["starts"], ptr["ends"], ptr["rco"],
                                       ptr["ws"], ws_bytes, dev_ptr(status), None))
    for name, (whole, _) in bufs.items():
        assert _guards_hold(whole, 777.0 if name == "chunks" else -7), "written outside " + name
    host = {k: v[1].cpu().numpy() for k, v in bufs.items()}
    return host["chunks"].reshape(chunk, total, 1), host["starts"], host["ends"], host["rco"], int(status.item())


SLACK = 16      # characters / rows nobody owns behind the last read's room


def call_dev(path, err, starts, ends, rco, stride, dev, scale=1.0, offset=0.0, room=None, alphabet=b"ACGT",
             read_scale=None, want_status=0):
    """tk_basecall_call_dev on per-chunk paths (nrow, nchunks) -> [(seq, qual or None)] per read.  `room`: every read's
    room, by default all the rows of its chunks; nothing may have been written past a read's call."""
    import torch
    from taiyaki_amd import _lib
    nread = len(rco) - 1
    nrow, nch = path.shape
    if room is None:
        room = [nrow * int(rco[r + 1] - rco[r]) for r in range(nread)]
    out_off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    seq = torch.full((int(out_off[-1]) + SLACK,), ord("."), dtype=torch.uint8, device=dev)
    qual = torch.full_like(seq, ord("."))
    seqlen = torch.full((nread,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    tensors = [_dev(path, np.int64, dev), _dev(err, np.float32, dev) if err is not None else None,
               _dev(starts, np.int64, dev), _dev(ends, np.int64, dev), _dev(rco, np.int64, dev),
               _dev(read_scale, np.float32, dev) if read_scale is not None else None, _dev(out_off, np.int64, dev)]
    ok(_lib.basecall_lib().tk_basecall_call_dev(
        dev_ptr(tensors[0]), dev_ptr(tensors[1]), nrow - 1, nch, dev_ptr(tensors[2]), dev_ptr(tensors[3]),
        dev_ptr(tensors[4]), dev_ptr(tensors[5]), nread, stride, len(alphabet), alphabet, scale, offset,
        dev_ptr(tensors[6]), dev_ptr(seq), dev_ptr(qual), dev_ptr(seqlen), dev_ptr(status), None))
    seq, qual, seqlen = seq.cpu().numpy(), qual.cpu().numpy(), seqlen.cpu().numpy()
    assert int(status.item()) == want_status, (int(status.item()), want_status)
    res = []
    for r in range(nread):
        assert 0 <= seqlen[r] <= room[r], (r, seqlen[r], room[r])
        lo, hi = int(out_off[r]), int(out_off[r]) + int(seqlen[r])
        assert (seq[hi:int(out_off[r + 1])] == ord(".")).all()          # nothing written past the call
        assert (qual[hi:int(out_off[r + 1])] == ord(".")).all()
        res.append((seq[lo:hi].tobytes().decode(), qual[lo:hi].tobytes().decode() if err is not None else None))
    assert (seq[int(out_off[-1]):] == ord(".")).all() and (qual[int(out_off[-1]):] == ord(".")).all()
    if err is None:
        assert (qual == ord(".")).all()                                 # errprobs NULL: qual untouched
    return res


STITCH_SENTINEL = np.uint32(0xFFFFFFFF)


def stitch_scores_dev(trans, starts, ends, rco, stride, rooms, dev, read_scale=None):
    """tk_basecall_stitch_scores_dev on trans (nblk, nchunks, S), given and returned as uint32 bit patterns ->
    (every read's rows, status): nrows[r] rows from row_off[r]; nothing may have been written behind them."""
    import torch
    from taiyaki_amd import _lib
    nblk, nch, S = trans.shape
    nread = len(rco) - 1
    row_off = np.concatenate([[0], np.cumsum(rooms)]).astype(np.int64)
    total = int(row_off[-1])
    out = _dev(np.full((total + SLACK, S), STITCH_SENTINEL, dtype=np.uint32).view(np.int32), np.int32, dev)
    nrows = torch.full((nread,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    t = [_dev(trans.view(np.int32), np.int32, dev), _dev(starts, np.int64, dev), _dev(ends, np.int64, dev),
         _dev(rco, np.int64, dev), _dev(read_scale, np.float32, dev) if read_scale is not None else None,
         _dev(row_off, np.int64, dev)]
    ok(_lib.basecall_lib().tk_basecall_stitch_scores_dev(
        dev_ptr(t[0]), nblk, nch, S, dev_ptr(t[1]), dev_ptr(t[2]), dev_ptr(t[3]), dev_ptr(t[4]), nread, stride,
        dev_ptr(t[5]), total, dev_ptr(out), dev_ptr(nrows), dev_ptr(status), None))
    out, nrows = out.cpu().numpy().view(np.uint32), nrows.cpu().numpy()
    res = []
    for r in range(nread):
        assert 0 <= nrows[r] <= rooms[r], (r, nrows[r], rooms[r])
        lo, hi = int(row_off[r]), int(row_off[r]) + int(nrows[r])
        assert (out[hi:int(row_off[r + 1])] == STITCH_SENTINEL).all()
        res.append(out[lo:hi])
    assert (out[total:] == STITCH_SENTINEL).all()
    return res, int(status.item())


MODS_SENTINEL = np.uint32(0xDEADBEEF)


def mod_weights_dev(path, weights, starts, ends, rco, stride, can_nmods, rooms, dev, read_scale=None):
    """tk_basecall_mod_weights_dev on paths (nblk + 1, nchunks) and weights (nblk, nchunks, ncat) ->
    (every read's rows as float32 (seqlen, nmod), status); nothing may have been written behind them."""
    import torch
    from taiyaki_amd import _lib
    nread, nmod, nch = len(rco) - 1, sum(can_nmods), path.shape[1]
    out_off = np.concatenate([[0], np.cumsum(rooms)]).astype(np.int64)
    total = int(out_off[-1])
    mods = _dev(np.full((total + SLACK, nmod), MODS_SENTINEL, dtype=np.uint32).view(np.int32), np.int32, dev)
    seqlen = torch.full((nread,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    t = [_dev(path, np.int64, dev), _dev(weights, np.float32, dev), _dev(starts, np.int64, dev), _dev(ends, np.int64, dev),
         _dev(rco, np.int64, dev), _dev(read_scale, np.float32, dev) if read_scale is not None else None,
         _dev(out_off, np.int64, dev)]
    ok(_lib.basecall_lib().tk_basecall_mod_weights_dev(
        dev_ptr(t[0]), dev_ptr(t[1]), path.shape[0] - 1, nch, dev_ptr(t[2]), dev_ptr(t[3]), dev_ptr(t[4]), dev_ptr(t[5]),
        nread, stride, len(can_nmods), (ctypes.c_int * len(can_nmods))(*can_nmods), dev_ptr(t[6]), dev_ptr(mods),
        dev_ptr(seqlen), dev_ptr(status), None))
    mods, seqlen = mods.cpu().numpy().view(np.uint32), seqlen.cpu().numpy()
    res = []
    for r in range(nread):
        assert 0 <= seqlen[r] <= rooms[r], (r, seqlen[r], rooms[r])
        lo, hi = int(out_off[r]), int(out_off[r]) + int(seqlen[r])
        assert (mods[hi:int(out_off[r + 1])] == MODS_SENTINEL).all()
        res.append(mods[lo:hi].view(np.float32))
    assert (mods[total:] == MODS_SENTINEL).all()
    return res, int(status.item())


def columnwise(dev):
    import torch

    class Columnwise(torch.nn.Module):
        """A stand-in network whose output column depends on its input column alone, through elementwise and
        strided-slice operations only (no GEMM): regrouping columns cannot change a bit of its output."""

        def __init__(self):
            super().__init__()
            self.w = torch.nn.Parameter(torch.linspace(-2.0, 2.0, 40))
            self.b = torch.nn.Parameter(torch.cos(torch.arange(40.0)))

        def forward(self, x):                                   # (T, N, 1) -> (ceil(T / 5), N, 40)
            y = x[::5]
            z = y * self.w + self.b
            return 5.0 * torch.tanh(z + 0.25 * torch.sin(3.0 * y * y))

    return Columnwise().to(dev)


# ----------------------------------------------------------------------------------------------------------------------
# median / MAD: signals for every branch of the radix selection
# ----------------------------------------------------------------------------------------------------------------------
def _seed(*key):
    return zlib.crc32(repr(key).encode())


MEDMAD_N = (2, 3, 4, 255, 256, 257, 511, 512, 513, 4097, 65537)
MEDMAD_FAMILIES = ("neg", "mix", "wide", "sub", "zeros", "two")


def medmad_cases():
    """[(family, n)]; `two` has n / 2 of each value, so it exists at even n only."""
    return [(f, n) for f in MEDMAD_FAMILIES for n in MEDMAD_N if f != "two" or n % 2 == 0]


def medmad_signal(family, n, salt=0):
    """neg: every key takes the sign-set branch.  mix: both branches, a median near 0.  wide: ten to the +-30, either
    sign, so the lanes of a wave fall into different leading bins.  sub: subnormals.  zeros: a fifth +0.0 and a tenth
    -0.0 among normal deviates, so the median is a zero (fewer than half are: the MAD is not).  two: n / 2 of -1.5 and of
    2.25: median 0.375, every deviation 1.875.  fixture: what tests/basecall_support.signal draws, without the drift."""
    rs = np.random.RandomState(_seed(family, n, salt))
    if family == "neg":
        x = -90.0 - 12.0 * rs.standard_normal(n)
    elif family == "mix":
        x = 3.0 * rs.standard_normal(n)
    elif family == "wide":
        x = rs.choice([-1.0, 1.0], size=n) * 10.0 ** rs.uniform(-30.0, 30.0, size=n)
    elif family == "sub":
        x = 1e-41 * rs.standard_normal(n)
    elif family == "zeros":
        x, where = rs.standard_normal(n), rs.permutation(n)
        x[where[:n // 5]] = 0.0
        x[where[n // 5:n // 5 + n // 10]] = -0.0
    elif family == "two":
        assert n % 2 == 0
        x = np.repeat([-1.5, 2.25], n // 2)
        rs.shuffle(x)
    else:
        assert family == "fixture", family
        x = 90.0 + 12.0 * rs.standard_normal(n)
    return x.astype(np.float32)


def med_mad_f32(x):
    """clipping.med_mad with the factor handed over as float32 -> (med, np.float32(1.4826) * spread), float32 scalars"""
    from taiyaki_amd import clipping
    med, mad = clipping.med_mad(np.asarray(x, dtype=np.float32), factor=np.float32(1.4826))
    return np.float32(med), np.float32(mad)


def radix_key(x):
    """The selection's order-preserving key (csrc/basecall_kernels.hip, key_of): of x + 0, so that -0 keys as +0"""
    u = (np.asarray(x, dtype=np.float32) + np.float32(0.0)).view(np.uint32)
    return np.where(u >> 31 != 0, ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def parting_pass(a, b):
    """The radix pass (0: the leading byte .. 3) at which the keys of a and b fall into different bins"""
    ka, kb = (int(k) for k in radix_key([a, b]))
    assert ka != kb
    return 3 - ((ka ^ kb).bit_length() - 1) // 8


_BITS = lambda u: np.array([u], dtype=np.uint32).view(np.float32)[0]  # noqa: E731
# the two middle values of an even-length read: they differ first in radix byte 0, 1, 2, 3
PARTING_PAIRS = ((np.float32(-1.0), np.float32(1.0)), (_BITS(0x3f800000), _BITS(0x3fc00000)),
                 (np.float32(1.0), _BITS(0x3f802000)), (np.float32(1.0), np.nextafter(np.float32(1.0), np.float32(2.0))))


def parting_signal(which):
    """1000 values: 499 from (-200, -100), the pair, 499 from (100, 200), shuffled"""
    rs = np.random.RandomState(_seed("parting", which))
    x = np.concatenate([rs.uniform(-200.0, -100.0, size=499), PARTING_PAIRS[which], rs.uniform(100.0, 200.0, size=499)])
    rs.shuffle(x)
    return x.astype(np.float32)


def refused_signals():
    """name -> a read the kernel refuses: med = mad = NaN, TK_STATUS_BAD_SIGNAL"""
    tied = medmad_signal("mix", 101, "tied")
    tied[:51] = np.float32(-2.5)                                # more than half of the values equal: MAD 0
    ninf = medmad_signal("neg", 300, "ninf")
    ninf[123] = -np.inf
    return {"empty": np.zeros(0, dtype=np.float32), "tied": tied, "ninf": ninf}


MEDMAD_BATCH = 300


@functools.lru_cache(maxsize=None)
def medmad_batch():
    """([signals], {index: name of a refused read}): MEDMAD_BATCH reads of every family and length, the parting reads,
    an empty read and the refused reads among them, so that read starts fall at odd offsets of the flat array."""
    cases = medmad_cases()
    sigs = [medmad_signal(*cases[(7 * r) % len(cases)], salt=("batch", r)) for r in range(MEDMAD_BATCH)]
    for which in range(len(PARTING_PAIRS)):
        sigs[31 + 60 * which] = parting_signal(which)
    refused = dict(zip((100, 101, 257), ("empty", "tied", "ninf")))
    for r, name in refused.items():
        sigs[r] = refused_signals()[name]
    return sigs, refused


# ----------------------------------------------------------------------------------------------------------------------
# chunk plan and gather past 256 reads
# ----------------------------------------------------------------------------------------------------------------------
PLAN_NREAD = (256, 257, 513, 1000)
PLAN_CHUNKING = ((64, 0), (100, 37), (129, 128), (200, 1))          # (chunk_size, overlap) in samples


def plan_lengths(nread, chunk, overlap):
    """Lengths that cycle through 0, 1, chunk - 1, chunk, chunk + 1, 2 chunk - overlap, 2 chunk - overlap + 1 and a
    seeded length up to 6 chunk, turned so that reads 255, 256 and 257 get chunk, chunk + 1 and 2 chunk - overlap."""
    rs = np.random.RandomState(_seed("plan", nread, chunk, overlap))
    cycle = [0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk - overlap, 2 * chunk - overlap + 1, None]
    lens = [cycle[(r + 4) % 8] for r in range(nread)]
    return np.array([int(rs.randint(6 * chunk + 1)) if n is None else n for n in lens], dtype=np.int64)


@functools.lru_cache(maxsize=None)
def plan_case(nread, chunk, overlap):
    """-> dict(signals, shift, scale) and what numpy gives for them: rco, starts, ends, chunks (chunk, total, 1).
    `neg` and `mix` signals by turns, a shift and a scale per read; a NaN shift or scale here and there: zero columns."""
    from taiyaki_amd import basecall, basecall_helpers
    lens = plan_lengths(nread, chunk, overlap)
    sigs = [medmad_signal("neg" if r % 2 else "mix", int(n), ("plan", nread, chunk, r)) for r, n in enumerate(lens)]
    shift = np.array([(-90.0 if r % 2 else 0.0) + 0.5 * (r % 7) for r in range(nread)], dtype=np.float32)
    scale = np.array([(12.0 if r % 2 else 3.0) + 0.25 * (r % 5) for r in range(nread)], dtype=np.float32)
    shift[5::11], scale[7::13] = np.nan, np.nan
    counts = basecall.chunk_counts(lens, chunk, overlap)
    starts, ends, cols = [np.zeros(0, dtype=np.int64)], [np.zeros(0, dtype=np.int64)], [np.zeros((chunk, 0, 1), "f4")]
    for r in np.flatnonzero(lens >= chunk):
        c, s, e = basecall_helpers.chunk_read(((sigs[r] - shift[r]) / scale[r]).astype("f4"), chunk, overlap)
        assert c.shape == (chunk, counts[r], 1)
        starts.append(s), ends.append(e), cols.append(c if not np.isnan(c).any() else np.zeros_like(c))
    return dict(signals=sigs, shift=shift, scale=scale, lens=lens, counts=counts,
                rco=np.concatenate([[0], np.cumsum(counts)]).astype(np.int64), starts=np.concatenate(starts),
                ends=np.concatenate(ends), chunks=np.concatenate(cols, axis=1))


# ----------------------------------------------------------------------------------------------------------------------
# the shared walk: read geometries, paths with dwell and forced moves
# ----------------------------------------------------------------------------------------------------------------------
WALK_STRIDE, WALK_NBLK, WALK_NCH = (1, 2, 5), (1, 2, 254, 255, 256, 257, 600), (0, 1, 2, 3, 5)
TILE = 256                                                      # rows of one tile of the walk (BC_THREADS)


def stitched_index(starts, ends, stride, nrow):
    """(row, chunk) of `path` (nrow, nchunks) for every stitched row of one read, as two index arrays"""
    keep = cuts(starts, ends, stride, nrow)
    rows = [np.arange(lo, max(hi, lo), dtype=np.int64) for lo, hi in keep]
    return np.concatenate(rows), np.concatenate([np.full(len(x), i, dtype=np.int64) for i, x in enumerate(rows)])


def walk_overlap(kind, chunk, rs):
    """kind 0: no overlap; 1: an odd one; 2: half a chunk -- in samples, below the chunk"""
    if kind == 1 and chunk >= 2:
        return 1 + 2 * int(rs.randint(chunk // 2))
    return chunk // 2 if kind == 2 else 0


def _dwell(n, nstate, rs):
    """n states: runs of 1 .. 6 equal states, neighbouring runs differ"""
    states = (rs.randint(nstate) + np.cumsum(rs.randint(1, nstate, size=n + 1))) % nstate
    return np.repeat(states, rs.randint(1, 7, size=n + 1))[:n].astype(np.int64)


def walk_read(r, stride, nblk, nbase):
    """Read r of a launch at (stride, nblk, nbase): nch by turns from WALK_NCH, the overlap kind by turns, a ragged last
    chunk; starts and ends from chunk_read on a signal of its length.  Forced into its stitched path, where the rows
    exist: moves at rows 255, 256 and 257 of the first cut that long (either side of the walk's tile boundary), a move
    exactly across one cut between two chunks and none across the next (which of the two comes first turns with r).
    `features` says what the finished path holds, whatever was intended."""
    from taiyaki_amd import basecall_helpers
    rs = np.random.RandomState(_seed("walk", r, stride, nblk, nbase))
    nch, nrow, chunk, nstate = WALK_NCH[r % 5], nblk + 1, nblk * stride, 2 * nbase
    overlap = walk_overlap((r // 5) % 3, chunk, rs)
    step = chunk - overlap
    read = dict(nch=nch, overlap=overlap, overlap_kind=(r // 5) % 3, refused=nch > 0 and r % 17 == 4, features=set())
    if nch == 0:
        return dict(read, starts=np.zeros(0, np.int64), ends=np.zeros(0, np.int64), path=np.zeros((nrow, 0), np.int64),
                    err=np.zeros((nrow, 0), np.float32), siglen=int(rs.randint(chunk)))
    siglen = chunk + (nch - 1) * step - (int(rs.randint(step)) if nch > 1 else 0)
    _, starts, ends = basecall_helpers.chunk_read(np.zeros(siglen, dtype=np.float32), chunk, overlap)
    assert len(starts) == nch
    rows, ci = stitched_index(starts, ends, stride, nrow)
    n = len(rows)
    st = _dwell(n, nstate, rs)
    first = np.concatenate([[0], np.flatnonzero(ci[1:] != ci[:-1]) + 1])       # stitched row of every cut's first row
    length = np.diff(np.concatenate([first, [n]]))
    for f, ln in zip(first, length):
        ks = [f + k for k in (TILE - 1, TILE, TILE + 1) if k < ln and f + k >= 1]
        if ks:
            st[ks[0] - 1:ks[-1] + 1] = (st[ks[0] - 1] + np.arange(len(ks) + 1)) % nstate
            break
    for j, b in enumerate(first[1:]):
        if j % 2 == (r // 5) % 2:
            st[b] = (st[b - 1] + 1 + rs.randint(nstate - 1)) % nstate           # a move exactly across the cut
        else:
            st[b] = st[b - 1]                                                   # none across this one
    move = np.concatenate([[False], st[1:] != st[:-1]])
    for f, ln in zip(first, length):
        read["features"] |= {"move at %d" % k for k in (TILE - 1, TILE, TILE + 1) if k < ln and move[f + k]}
    read["features"] |= {"move across a cut" if move[b] else "no move across a cut" for b in first[1:]}
    if nch > 1 and any(hi <= lo for lo, hi in cuts(starts, ends, stride, nrow)):
        read["features"].add("empty cut")
    path = rs.randint(nstate, size=(nrow, nch)).astype(np.int64)                # (the rows the cuts drop: anything)
    path[rows, ci] = st
    err = np.exp(rs.uniform(np.log(1e-6), np.log(0.5), size=(nrow, nch))).astype(np.float32)
    return dict(read, starts=np.asarray(starts, np.int64), ends=np.asarray(ends, np.int64), path=path, err=err,
                siglen=siglen, stitched=st)


@functools.lru_cache(maxsize=None)
def walk_launch(stride, nblk, nbase, nread):
    """`nread` reads of walk_read in one launch: reads without chunks and refused reads (a NaN scale) among the
    others.  -> dict(reads, path, err (nrow, nchunks), starts, ends, rco, scale, alphabet, qs, qo, want): want[r] is
    (sequence, quality string) of the numpy tail, ("", "") for a read without chunks or a refused one."""
    reads = [walk_read(r, stride, nblk, nbase) for r in range(nread)]
    alphabet = "ACGT"[:nbase]
    qs, qo = ((1.0, 0.0), (0.9, 0.3))[(nblk + stride) % 2]
    want = [("", "") if rd["nch"] == 0 or rd["refused"] else
            tail(rd["path"], rd["err"], rd["starts"], rd["ends"], stride, alphabet, qs, qo)[:2] for rd in reads]
    return dict(reads=reads, stride=stride, nblk=nblk, nbase=nbase, alphabet=alphabet, qs=qs, qo=qo, want=want,
                path=np.concatenate([rd["path"] for rd in reads], axis=1),
                err=np.concatenate([rd["err"] for rd in reads], axis=1),
                starts=np.concatenate([rd["starts"] for rd in reads]), ends=np.concatenate([rd["ends"] for rd in reads]),
                rco=np.concatenate([[0], np.cumsum([rd["nch"] for rd in reads])]).astype(np.int64),
                scale=np.array([np.nan if rd["refused"] else 1.0 for rd in reads], dtype=np.float32))


def walk_columns(launch, r):
    """(lo, hi, read_chunk_off) to launch read r alone: its own columns, or -- a read without chunks, and a launch needs
    a column -- column 0 of the launch, which read_chunk_off = [0, 0] gives to nobody"""
    lo, hi = int(launch["rco"][r]), int(launch["rco"][r + 1])
    return (lo, hi, np.array([0, hi - lo])) if hi > lo else (0, 1, np.array([0, 0]))


# ----------------------------------------------------------------------------------------------------------------------
# one whole call
# ----------------------------------------------------------------------------------------------------------------------
WHOLE_CALL = dict(stride=5, chunk_size=40, overlap=8, max_concurrent_chunks=16, fastq=True, pack=True)


@functools.lru_cache(maxsize=None)
def whole_call_reads(nread=300):
    """([signals], [None or the caller's own (shift, scale)]): reads of 0 .. 1500 samples, `neg`, `mix` and fixture-like
    by turns; every second read has the caller's parameters.  Read 100 has no samples."""
    rs = np.random.RandomState(_seed("whole call", nread))
    lens = rs.randint(0, 1501, size=nread)
    lens[100] = 0
    family = [("neg", (-90.0, 12.0)), ("mix", (0.25, 3.0)), ("fixture", (88.0, 11.5))]
    sigs = [medmad_signal(family[r % 3][0], int(n), ("whole call", r)) for r, n in enumerate(lens)]
    return sigs, [family[r % 3][1] if r % 2 else None for r in range(nread)]
