"""The basecaller's device glue beyond its eleven-read fixture (taiyaki_amd/csrc/basecall_kernels.hip, basecall_walk.h,
basecall_mods.hip), at the C ABI of include/taiyaki_amd_basecall.h.

1. tk_signal_med_mad_dev on every branch of the radix selection: negative keys, zero crossings, -0, subnormals, waves
   whose lanes fall into different leading bins, the pass at which the two middle ranks part, refused reads, 300 reads
   in one launch.
2. tk_basecall_gather_chunks_dev past 256 reads (the plan's carry between blocks of 256), and with a `total_chunks`
   that disagrees with the lengths, every buffer between sentinels.
3. The shared walk under tk_basecall_call_dev, tk_basecall_stitch_scores_dev and tk_basecall_mod_weights_dev: moves on
   and beside the 256-row tile boundary, across a cut and not, empty cuts, reads without chunks and refused reads
   among the others, a room that fits exactly and one that is one short, stride 1, 300 reads in one launch.
4. One `Basecaller.call` of 300 reads against one call per read.

The references are the project's numpy restatements, which the CPU tests of tests/test_basecall_reads.py and
tests/test_basecall_mods.py pin to the genuine reference: clipping.med_mad, basecall_helpers.chunk_read,
basecall.chunk_counts, bs.cuts / bs.tail, ms.moves_to_mods.  Every comparison is one of bits, with two exceptions:
a median of zero compares by value (the kernel selects on x + 0 and returns +0 where numpy may return -0), and quality
characters follow the project's rule for the device's log10f (bs.qstrings_close).

The generators and the launches are in tests/basecall_support.py; the CPU tests here check that the generated inputs
hold what they are meant to hold."""
import itertools

import numpy as np
import pytest

from tests import basecall_support as bs
from tests import mods_support as ms


def _bits(x):
    return np.asarray(x, dtype=np.float32).tobytes()


def _same_median(got, want):
    """Bit-equal -- or both zero: the kernel returns +0 where numpy's median of zeros may be -0."""
    return _bits(got) == _bits(want) or (got == 0 and want == 0)


# ----------------------------------------------------------------------------------------------------------------------
# CPU: the generated inputs hold what they are meant to hold
# ----------------------------------------------------------------------------------------------------------------------
def test_parting_pairs_part_at_the_intended_pass():
    for which, (a, b) in enumerate(bs.PARTING_PAIRS):
        assert a < b and bs.parting_pass(a, b) == which
        x = np.sort(bs.parting_signal(which))
        assert len(x) == 1000 and _bits(x[499:501]) == _bits([a, b]) and x[498] < -100 and x[501] > 100
    assert [hex(int(np.float32(v).view(np.uint32))) for v in bs.PARTING_PAIRS[2]] == ["0x3f800000", "0x3f802000"]
    # the key is the order of the floats, and -0 keys as +0
    x = np.concatenate([bs.medmad_signal(f, 257) for f in ("neg", "mix", "wide", "sub", "zeros")])
    order = np.argsort(x, kind="stable")
    assert (np.diff(bs.radix_key(x)[order].astype(np.int64)) >= 0).all()
    assert (np.diff(bs.radix_key(x)[order].astype(np.int64)) > 0).sum() == len(np.unique(x)) - 1
    assert bs.radix_key(np.float32(-0.0)) == bs.radix_key(np.float32(0.0)) == 0x80000000


def test_med_mad_families_are_what_they_claim():
    for family, n in bs.medmad_cases():
        x = bs.medmad_signal(family, n)
        med, mad = bs.med_mad_f32(x)
        assert x.dtype == np.float32 and len(x) == n and np.isfinite(x).all()
        assert mad > 0 and np.isfinite(mad) and mad.dtype == np.float32, (family, n)      # a value is expected
        lead = bs.radix_key(x[:64]) >> 24                                                   # the first wave's bins
        if family == "neg":
            assert (x < 0).all() and (lead < 0x80).all()
        elif family == "mix":
            assert n < 4 or ((x < 0).any() and (x > 0).any())
        elif family == "wide":
            assert n < 255 or len(np.unique(lead)) >= 32
        elif family == "sub":
            assert (np.abs(x) < np.finfo(np.float32).tiny).all() and np.count_nonzero(x) > 0.99 * n
        elif family == "zeros":
            zero = x == 0
            assert 2 * zero.sum() < n
            if n >= 255:
                assert med == 0 and (np.signbit(x) & zero).any() and (~np.signbit(x) & zero).any()
        elif family == "two":
            assert med == np.float32(0.375) and _bits(mad) == _bits(np.float32(1.4826) * np.float32(1.875))
    for which in range(len(bs.PARTING_PAIRS)):
        assert bs.med_mad_f32(bs.parting_signal(which))[1] > 0
    refused = bs.refused_signals()
    assert len(refused["empty"]) == 0 and bs.med_mad_f32(refused["tied"])[1] == 0
    assert np.isneginf(refused["ninf"]).sum() == 1 and np.isfinite(refused["ninf"]).sum() == len(refused["ninf"]) - 1
    sigs, bad = bs.medmad_batch()
    assert len(sigs) == bs.MEDMAD_BATCH == 300 and sorted(bad) == [100, 101, 257]
    assert all(bs.med_mad_f32(x)[1] > 0 for r, x in enumerate(sigs) if r not in bad)
    starts = np.cumsum([len(x) for x in sigs])[:-1]
    assert (starts % 2 == 1).sum() > 50 and (starts % 64 != 0).sum() > 250           # reads start at odd offsets
    assert {len(x) for x in sigs} >= set(bs.MEDMAD_N)


@pytest.mark.parametrize("chunk, overlap", bs.PLAN_CHUNKING)
@pytest.mark.parametrize("nread", bs.PLAN_NREAD)
def test_plan_lengths_reach_reads_255_to_257(nread, chunk, overlap):
    from taiyaki_amd import basecall
    lens = bs.plan_lengths(nread, chunk, overlap)
    counts = basecall.chunk_counts(lens, chunk, overlap)
    assert len(lens) == nread and (counts[255:258] > 0).all() and lens.max() <= 6 * chunk
    assert lens[255:258].tolist() == [chunk, chunk + 1, 2 * chunk - overlap][:nread - 255]
    assert set(lens) >= {0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk - overlap, 2 * chunk - overlap + 1}
    c = bs.plan_case(nread, chunk, overlap)
    assert c["chunks"].shape == (chunk, counts.sum(), 1) and len(c["starts"]) == len(c["ends"]) == counts.sum()
    # the running count that block 1 (reads 256 ..) starts from is not 0, and reads of every kind lie behind it
    assert c["rco"][256] > 0 and (nread == 256 or c["rco"][-1] > c["rco"][256])
    nan = np.isnan(c["shift"]) | np.isnan(c["scale"])
    assert (nan & (counts > 0)).any() and not nan[255:258].any()
    print("nread %d chunk %d overlap %d: %d chunks" % (nread, chunk, overlap, counts.sum()))


WALK_GEOMETRY = [(stride, nblk, 2 if i % 2 else 4)
                 for i, (stride, nblk) in enumerate(itertools.product(bs.WALK_STRIDE, bs.WALK_NBLK))]
WALK_300 = [(5, 600, 4), (1, 257, 2), (2, 256, 4)]
WALK_LAUNCHES = [g + (40,) for g in WALK_GEOMETRY] + [g + (300,) for g in WALK_300]


def test_walk_generator_forces_its_moves():
    seen = set()
    for stride, nblk, nbase in WALK_GEOMETRY:
        L = bs.walk_launch(stride, nblk, nbase, 40)
        reads = L["reads"]
        feats = set().union(*(rd["features"] for rd in reads))
        seen |= feats
        assert {"move across a cut", "no move across a cut"} <= feats, (stride, nblk)
        for k in (255, 256, 257):                       # a cut of nblk + 1 rows has the row: the move is there
            assert ("move at %d" % k in feats) == (k <= nblk), (stride, nblk, k)
        assert {rd["nch"] for rd in reads} == set(bs.WALK_NCH)
        assert any(rd["refused"] for rd in reads) and not all(rd["refused"] for rd in reads if rd["nch"])
        has = [rd["nch"] > 0 and not rd["refused"] for rd in reads]
        assert any(has[i - 1] and not has[i] and has[i + 1] for i in range(1, 39))      # none between two that have
        chunk = nblk * stride
        assert {rd["overlap_kind"] for rd in reads if rd["nch"] > 1} == {0, 1, 2}      # none, odd, half a chunk
        for rd in reads:
            assert 0 <= rd["overlap"] < chunk
            assert rd["overlap"] == (0, rd["overlap"], chunk // 2)[rd["overlap_kind"]]
            assert rd["overlap_kind"] != 1 or chunk < 2 or rd["overlap"] % 2 == 1
        assert L["err"].min() >= 1e-6 and L["err"].max() <= 0.5 and L["path"].max() == 2 * nbase - 1
        # dwell: runs of 1 .. 6 equal states, but for the forced rows
        st = next(rd["stitched"] for rd in reads if rd["nch"] == 1 and not rd["refused"])
        runs = np.diff(np.flatnonzero(np.concatenate([[True], st[1:] != st[:-1], [True]])))
        assert runs.max() <= 6 and (nblk < 100 or (runs > 1).mean() > 0.5)
        # ragged last chunks, as chunk_read makes them
        assert nblk * stride < 2 or any(rd["nch"] > 1 and rd["ends"][-1] - rd["ends"][-2] < chunk - rd["overlap"]
                                        for rd in reads)
    assert "empty cut" in seen
    L = bs.walk_launch(*WALK_300[0], 300)
    assert len(L["reads"]) == 300 and L["rco"][256] > 0 and sum(len(s) > 0 for s, _ in L["want"]) > 200


def test_whole_call_reads_can_call_200(oracle_mod):
    """The network's scores of every read's first chunk, on the CPU, and the oracle's Viterbi on them: a read whose path
    changes state calls a base.  (The device call decodes the posterior transition weights of all chunks; the GPU
    test asserts the count on its result.  This one says that the bound is within the reads' reach.)"""
    import torch
    net = bs.columnwise("cpu")
    sigs, params = bs.whole_call_reads()
    assert len(sigs) == 300 and [p is not None for p in params[:4]] == [False, True, False, True]
    assert min(map(len, sigs)) == 0 and 1400 < max(map(len, sigs)) <= 1500
    chunk = bs.WHOLE_CALL["chunk_size"] * bs.WHOLE_CALL["stride"]
    assert sum(len(x) >= chunk for x in sigs) > 200 and sum(0 < len(x) < chunk for x in sigs) > 10
    calling = 0
    for x, p in zip(sigs, params):
        shift, scale = p if p is not None else bs.med_mad_f32(x)
        if len(x) == 0 or not scale > 0:
            continue
        first = ((x - np.float32(shift)) / np.float32(scale)).astype("f4")[:chunk]
        with torch.no_grad():
            scores = net(torch.from_numpy(first)[:, None, None]).numpy()
        path = oracle_mod.flipflop_viterbi(scores)[2][:, 0]
        calling += bool((path[1:] != path[:-1]).any())
    print("%d of %d reads change state in their first chunk" % (calling, len(sigs)))
    assert calling >= 200


# ----------------------------------------------------------------------------------------------------------------------
# GPU 1: median / MAD
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("family, n", bs.medmad_cases())
def test_med_mad_on_every_branch_of_the_selection(gpu_device, family, n):
    x = bs.medmad_signal(family, n)
    want_med, want_mad = bs.med_mad_f32(x)
    med, mad, status = bs.med_mad_dev([x], gpu_device)
    assert status == 0
    assert _same_median(med[0], want_med), (family, n, med[0], want_med)
    assert _bits(mad[0]) == _bits(want_mad), (family, n, mad[0], want_mad)
    if family == "two":
        assert med[0] == np.float32(0.375)


@pytest.mark.gpu
@pytest.mark.parametrize("which", range(len(bs.PARTING_PAIRS)))
def test_med_mad_where_the_middle_ranks_part(gpu_device, which):
    x = bs.parting_signal(which)
    want_med, want_mad = bs.med_mad_f32(x)
    med, mad, status = bs.med_mad_dev([x], gpu_device)
    assert status == 0
    assert _same_median(med[0], want_med), (which, med[0], want_med)
    assert _bits(mad[0]) == _bits(want_mad), (which, mad[0], want_mad)


@pytest.mark.gpu
def test_med_mad_refuses_and_leaves_the_neighbours_alone(gpu_device):
    left, right = bs.medmad_signal("neg", 257), bs.medmad_signal("wide", 513)
    alone = [bs.med_mad_dev([x], gpu_device) for x in (left, right)]
    assert alone[0][2] == alone[1][2] == 0
    for name, bad in bs.refused_signals().items():
        med, mad, status = bs.med_mad_dev([bad], gpu_device)
        assert status == bs.BAD_SIGNAL and np.isnan(med[0]) and np.isnan(mad[0]), name
        med, mad, status = bs.med_mad_dev([left, bad, right], gpu_device)
        assert status == bs.BAD_SIGNAL and np.isnan(med[1]) and np.isnan(mad[1]), name
        assert _bits(med[[0, 2]]) == _bits([alone[0][0][0], alone[1][0][0]]), name
        assert _bits(mad[[0, 2]]) == _bits([alone[0][1][0], alone[1][1][0]]), name


@pytest.mark.gpu
def test_med_mad_300_reads_in_one_launch(gpu_device):
    sigs, bad = bs.medmad_batch()
    med, mad, status = bs.med_mad_dev(sigs, gpu_device)
    assert status == bs.BAD_SIGNAL
    for r, x in enumerate(sigs):
        if r in bad:
            assert np.isnan(med[r]) and np.isnan(mad[r]), (r, bad[r])
            continue
        want_med, want_mad = bs.med_mad_f32(x)
        assert _same_median(med[r], want_med) and _bits(mad[r]) == _bits(want_mad), (r, len(x), med[r], want_med)
    # bit for bit what every read gets alone
    sample = sorted(set(np.random.RandomState(5).choice(len(sigs), 40, replace=False)) | set(bad) | {0, 255, 256, 299})
    assert len(sample) >= 40
    for r in sample:
        m1, d1, s1 = bs.med_mad_dev([sigs[r]], gpu_device)
        assert s1 == (bs.BAD_SIGNAL if r in bad else 0)
        if r not in bad:
            assert _bits(m1[0]) == _bits(med[r]) and _bits(d1[0]) == _bits(mad[r]), r


# ----------------------------------------------------------------------------------------------------------------------
# GPU 2: chunk plan and gather past 256 reads
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("chunk, overlap", bs.PLAN_CHUNKING)
@pytest.mark.parametrize("nread", bs.PLAN_NREAD)
def test_chunk_plan_and_gather_past_256_reads(gpu_device, nread, chunk, overlap):
    c = bs.plan_case(nread, chunk, overlap)
    chunks, starts, ends, rco, status = bs.gather_dev(c["signals"], c["shift"], c["scale"], gpu_device, chunk, overlap)
    assert status == 0
    np.testing.assert_array_equal(rco, c["rco"])                # the cumulative sum of basecall.chunk_counts
    np.testing.assert_array_equal(starts, c["starts"])          # chunk_read's, read after read
    np.testing.assert_array_equal(ends, c["ends"])
    assert chunks.shape == c["chunks"].shape
    wrong = np.flatnonzero((chunks.view(np.uint32) != c["chunks"].view(np.uint32)).any(axis=(0, 2)))
    assert len(wrong) == 0, "first differing column %d (read %d)" % (wrong[0], np.searchsorted(rco, wrong[0], "right") - 1)


@pytest.mark.gpu
@pytest.mark.parametrize("chunk, overlap", bs.PLAN_CHUNKING)
@pytest.mark.parametrize("nread", (257, 1000))
def test_chunk_plan_with_a_total_that_disagrees(gpu_device, nread, chunk, overlap):
    c = bs.plan_case(nread, chunk, overlap)
    total = int(c["rco"][-1])
    args = (c["signals"], c["shift"], c["scale"], gpu_device, chunk, overlap)
    # two more than the lengths give: flagged, the surplus columns zero, every other column as before
    chunks, starts, ends, rco, status = bs.gather_dev(*args, total=total + 2)
    assert status == bs.CHUNK_PLAN
    assert not chunks[:, total:].view(np.uint32).any() and not starts[total:].any() and not ends[total:].any()
    assert chunks[:, :total].tobytes() == c["chunks"].tobytes()
    np.testing.assert_array_equal(starts[:total], c["starts"])
    np.testing.assert_array_equal(ends[:total], c["ends"])
    np.testing.assert_array_equal(rco, c["rco"])
    # two fewer: flagged, nothing outside the smaller buffers (gather_dev checks the sentinels around each of them),
    # the columns that exist as before
    chunks, starts, ends, rco, status = bs.gather_dev(*args, total=total - 2)
    assert status == bs.CHUNK_PLAN and chunks.shape == (chunk, total - 2, 1)
    assert chunks.tobytes() == c["chunks"][:, :total - 2].tobytes()
    np.testing.assert_array_equal(starts, c["starts"][:total - 2])
    np.testing.assert_array_equal(ends, c["ends"][:total - 2])
    np.testing.assert_array_equal(rco, c["rco"])


# ----------------------------------------------------------------------------------------------------------------------
# GPU 3: the shared walk
# ----------------------------------------------------------------------------------------------------------------------
def _walk_sample(nread, seed):
    """At least 30 reads of a 300-read launch, the reads around the 256th and the last among them"""
    return sorted(set(np.random.RandomState(seed).choice(nread, 30, replace=False)) | {0, 255, 256, 257, nread - 1})


def _call(L, dev, cols=None, **kw):
    lo, hi, rco, scale = (0, L["path"].shape[1], L["rco"], L["scale"]) if cols is None else cols
    return bs.call_dev(L["path"][:, lo:hi], L["err"][:, lo:hi], L["starts"][lo:hi], L["ends"][lo:hi], rco, L["stride"], dev,
                       L["qs"], L["qo"], alphabet=L["alphabet"].encode(), read_scale=scale, **kw)


def _alone(L, r):
    lo, hi, rco = bs.walk_columns(L, r)
    return lo, hi, rco, L["scale"][r:r + 1]


@pytest.mark.gpu
@pytest.mark.parametrize("stride, nblk, nbase, nread", WALK_LAUNCHES)
def test_call_kernel_on_the_walk(gpu_device, stride, nblk, nbase, nread):
    """Sequences and lengths exactly the numpy tail's.  Quality characters by the project's rule for the device's
    log10f (bs.qstrings_close): per read equal length and no character more than one step off; the rule's `fewer than
    1 % differ` is taken over the launch's characters, since some reads here have fewer than a hundred."""
    L = bs.walk_launch(stride, nblk, nbase, nread)
    got = _call(L, gpu_device)                                  # (status 0, nothing written past a call: call_dev)
    for r, ((seq, q), (wseq, wq)) in enumerate(zip(got, L["want"])):
        assert seq == wseq and len(q) == len(wq), r
    allq, allw = "".join(q for _, q in got), "".join(q for _, q in L["want"])
    ndiff = sum(a != b for a, b in zip(allq, allw))
    print("stride %d nblk %d nbase %d, %d reads: %d bases, %d quality characters differ from numpy's"
          % (stride, nblk, nbase, nread, len(allq), ndiff))
    assert len(allq) > 0
    diff = np.abs(np.frombuffer(allq.encode(), np.uint8).astype(int) - np.frombuffer(allw.encode(), np.uint8))
    assert diff.max() <= 1 and bs.qstrings_close(allq, allw)
    if nread > 40:                                              # every read as it is alone
        for r in _walk_sample(nread, 11):
            assert _call(L, gpu_device, _alone(L, r)) == [got[r]], r
        return
    for r in range(nread):                                      # a room that fits exactly, and one that is one short
        n = len(got[r][0])
        assert _call(L, gpu_device, _alone(L, r), room=[n]) == [got[r]], r
        if n > 0:
            short = _call(L, gpu_device, _alone(L, r), room=[n - 1], want_status=bs.CHUNK_PLAN)
            assert short == [(got[r][0][:n - 1], got[r][1][:n - 1])], r


STITCH_S = 40


def _trans_bits(nblk, nchunks):
    """Scores whose bits say where they sit: 0x3f000000 + the flat index of (row, chunk, column), all different"""
    assert nblk * nchunks * STITCH_S < 1 << 24
    return (np.uint32(0x3f000000) + np.arange(nblk * nchunks * STITCH_S, dtype=np.uint32)).reshape(nblk, nchunks, STITCH_S)


@pytest.mark.gpu
@pytest.mark.parametrize("stride, nblk, nbase, nread", WALK_LAUNCHES)
def test_stitch_scores_kernel_on_the_walk(gpu_device, stride, nblk, nbase, nread):
    L = bs.walk_launch(stride, nblk, nbase, nread)
    trans = _trans_bits(nblk, L["path"].shape[1])
    want = []
    for r, rd in enumerate(L["reads"]):
        if rd["nch"] == 0 or rd["refused"]:
            want.append(np.zeros((0, STITCH_S), dtype=np.uint32))
            continue
        rows, ci = bs.stitched_index(rd["starts"], rd["ends"], stride, nblk)        # (the scores have nblk rows)
        want.append(trans[rows, int(L["rco"][r]) + ci])
    rooms = [len(w) + r % 3 for r, w in enumerate(want)]        # the stitched row count, and a little more for some
    got, status = bs.stitch_scores_dev(trans, L["starts"], L["ends"], L["rco"], stride, rooms, gpu_device, L["scale"])
    assert status == 0
    for r, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), r   # nrows, and the rows bit for bit
    assert sum(len(w) for w in want) > 0
    for r in (_walk_sample(nread, 12) if nread > 40 else ()):
        lo, hi, rco, scale = _alone(L, r)
        one, status = bs.stitch_scores_dev(np.ascontiguousarray(trans[:, lo:hi]), L["starts"][lo:hi], L["ends"][lo:hi], rco,
                                           stride, [rooms[r]], gpu_device, scale)
        assert status == 0 and np.array_equal(one[0], got[r]), r


@pytest.mark.gpu
@pytest.mark.parametrize("can_nmods", [(1, 1, 0, 0), (2, 0, 1, 0)])
@pytest.mark.parametrize("stride, nblk, nbase, nread", [g for g in WALK_LAUNCHES if g[2] == 4])
def test_mod_weights_kernel_on_the_walk(gpu_device, stride, nblk, nbase, nread, can_nmods):
    """The rule of tests/test_basecall_mods.py: a move at stitched row k takes the weight row of stitched row k - 1, from
    the chunk that holds it (ms.moves_to_mods on the stitched weight rows)."""
    L = bs.walk_launch(stride, nblk, nbase, nread)
    nch = L["path"].shape[1]
    w = ms.weights((nblk, nch, nbase + sum(can_nmods)), 81)
    want = []
    for r, rd in enumerate(L["reads"]):
        if rd["nch"] == 0 or rd["refused"]:
            want.append(np.zeros((0, sum(can_nmods)), dtype=np.float32))
            continue
        rows, ci = bs.stitched_index(rd["starts"], rd["ends"], stride, nblk + 1)
        sp = rd["path"][rows, ci]
        assert np.array_equal(sp, rd["stitched"]) and (rows[:-1] < nblk).all()
        want.append(ms.moves_to_mods(w[np.minimum(rows, nblk - 1), int(L["rco"][r]) + ci], sp, can_nmods))
    rooms = [(nblk + 1) * rd["nch"] for rd in L["reads"]]
    got, status = bs.mod_weights_dev(L["path"], w, L["starts"], L["ends"], L["rco"], stride, can_nmods, rooms, gpu_device,
                                     L["scale"])
    assert status == 0
    called = bs.call_dev(L["path"], None, L["starts"], L["ends"], L["rco"], stride, gpu_device, read_scale=L["scale"])
    for r, (g, x) in enumerate(zip(got, want)):
        assert len(g) == len(called[r][0]) == len(L["want"][r][0]), r          # seqlen: the call kernel's
        assert ms.same_bits(g, x), r
    assert sum(len(x) for x in want) > 0
    for r in (_walk_sample(nread, 13) if nread > 40 else ()):
        lo, hi, rco, scale = _alone(L, r)
        one, status = bs.mod_weights_dev(L["path"][:, lo:hi], w[:, lo:hi], L["starts"][lo:hi], L["ends"][lo:hi], rco,
                                         stride, can_nmods, [rooms[r]], gpu_device, scale)
        assert status == 0 and one[0].tobytes() == got[r].tobytes(), r


# ----------------------------------------------------------------------------------------------------------------------
# GPU 4: one whole call of 300 reads
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_one_call_of_300_reads_equals_one_call_per_read(gpu_device):
    from taiyaki_amd import basecall
    sigs, params = bs.whole_call_reads()
    caller = basecall.Basecaller(bs.columnwise(gpu_device), **bs.WHOLE_CALL)
    got = caller.call(sigs, params)
    assert len(got) == len(sigs) == 300
    for x, (seq, q, nsample) in zip(sigs, got):
        assert len(q) == len(seq) and nsample == len(x) and set(seq) <= set("ACGT")
    calling = sum(len(seq) > 0 for seq, _, _ in got)
    print("%d of %d reads call a base, %d bases in all" % (calling, len(got), sum(len(seq) for seq, _, _ in got)))
    assert calling >= 200                                       # (the equality below is not one of empty strings)
    sample = sorted(set(np.random.RandomState(17).choice(len(sigs), 40, replace=False)) | {255, 256, 257, len(sigs) - 1})
    assert len(sample) >= 40
    for r in sample:
        assert caller.call([sigs[r]], [params[r]]) == [got[r]], r
