"""Chunks of a fixed number of bases (include/taiyaki_amd_chunks_seqlen.h) on the host: the numpy restatement
(tests/chunks_seqlen_support.py) against the fixture the genuine reference wrote (tests/golden/chunks_seqlen.npz), the
product's candidate draw order and capacity bound against the same fixture, the header, the library and the binding, and
what is refused before any device is touched."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from taiyaki_amd import _lib, mapped_signal as ms
from tests import chunks_seqlen_support as support
from tests.chunks_seqlen_support import REASONS, ReplayRng, fields, filter_dict, same, same_bits
from tests.golden.make_golden_chunks_seqlen import FORMS, SPECS, spec_reads

ENTRIES = {"tk_chunks_seqlen_locate_dev", "tk_chunks_seqlen_gather_dev"}
CASES = [(name, form) for name in sorted(SPECS) for form in FORMS]


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "chunks_seqlen.npz"))


def restated_filter_parameters(reads, spec, form, rng):
    """chunk_selection.sample_filter_parameters in either form: (median, mad)"""
    nofilter = filter_dict(spec, on=False)
    if form == "smp":       # chunks of `bases` SAMPLES: the restatement the sample-length producer is pinned to
        from oracle import chunks as oc
        return oc.sample_filter_parameters(reads, spec["nsample"], spec["bases"], nofilter, rng)
    limit = int(spec["nsample"] / spec["min_pass"])
    # (drawn one by one: the reference's loop stops drawing with its last accepted chunk)
    lazy = (support.candidates_from_rng(reads, 1, spec["bases"], rng)[0] for _ in range(limit))
    chunks, _, _ = support.sample_chunks(reads, spec["nsample"], spec["bases"], nofilter, lazy)
    return support.med_mad(support.mean_dwells(chunks))


@pytest.mark.parametrize("name, form", CASES)
def test_restatement_is_the_reference(golden, name, form):
    spec, g = SPECS[name], fields(golden, name, form)
    reads = spec_reads(spec)
    med, mad = restated_filter_parameters(reads, spec, form, ReplayRng(g["draws_filter"]))
    assert (med, mad) == tuple(g["median_mad"])
    fp = filter_dict(spec, med, mad)
    limit = int(spec["nwant"] / spec["min_pass"])
    cand = support.candidates_from_rng(reads, limit, spec["bases"], ReplayRng(g["draws_batch"]))
    chunks, counts, attempts = support.sample_chunks(reads, spec["nwant"], spec["bases"], fp, cand)
    assert [counts.get(k, 0) for k in REASONS] == list(g["rejections"])
    assert attempts == int(g["rejections"].sum())
    assert [c["read"] for c in chunks] == list(g["chunk_read"])
    assert [c["start"] for c in chunks] == list(g["chunk_start"])
    assert [c["max_dwell"] for c in chunks] == list(g["chunk_maxdwell"])
    assert [len(c["current"]) for c in chunks] == list(g["chunk_siglen"])
    for tag, rev in (("fwd", False), ("rev", True)):
        seq_embed, signal, siglens, seqs = support.assemble_batch(chunks, reverse=rev)
        assert same_bits(signal, g["signal_" + tag]) and same(siglens, g["chunk_siglen"])
        assert same(seqs, g["seqs_" + tag]) and same_bits(seq_embed, g["embed_" + tag])


def test_fixture_holds_what_it_was_made_for(golden):
    """Every rejection the sequence-length producer can give occurs, a batch is short, one is empty."""
    seen = np.sum([golden["%s/%s/rejections" % c] for c in CASES], axis=0)
    assert all(seen[REASONS.index(k)] > 0 for k in ("pass", "emptysignal", "tooshort", "pathbuffer", "meandwell",
                                                     "maxdwell"))
    assert seen[REASONS.index("emptysequence")] == 0 and seen[REASONS.index("nullmapping")] == 0
    assert len(golden["r30b150/seq/chunk_read"]) < SPECS["r30b150"]["nwant"]
    assert len(golden["r20b1/smp/chunk_read"]) == 0 and set(golden["r20b1/seq/chunk_maxdwell"]) == {1}
    assert len(golden["r6b100/seq/chunk_read"]) > SPECS["r6b100"]["nreads"]


@pytest.mark.parametrize("name, form", CASES)
def test_candidate_draw_order_is_the_reference(golden, name, form):
    """The product's host-side draws ask numpy for the reference's bounds in the reference's order (the replay asserts
    each bound) and give the restatement's candidates."""
    spec, g = SPECS[name], fields(golden, name, form)
    reads = spec_reads(spec)
    limit = int(spec["nwant"] / spec["min_pass"])
    regions = ms.mapped_reference_regions(reads)
    assert [tuple(x) for x in regions] == [support.mapped_reference_region(r) for r in reads]
    rng = ReplayRng(g["draws_batch"])
    cr, cs = ms.draw_reference_sequence_candidates(regions, limit, spec["bases"], rng)
    assert rng.k == len(g["draws_batch"])
    want = support.candidates_from_rng(reads, limit, spec["bases"], ReplayRng(g["draws_batch"]))
    assert [(int(a), int(b)) for a, b in zip(cr, cs)] == want
    seq_r, _ = ms.draw_reference_sequence_candidates(regions, 5, 10 ** 9, None, select_strands_randomly=False,
                                                     first_strand_index=len(reads) - 2)
    assert list(seq_r) == [len(reads) - 2, len(reads) - 1, 0, 1, 2]


@pytest.mark.parametrize("name, form", CASES)
def test_capacity_bound_holds_every_recorded_chunk(golden, name, form):
    spec, g = SPECS[name], fields(golden, name, form)
    med, mad = g["median_mad"]
    fp = ms.FILTER_PARAMETERS(**filter_dict(spec, float(med), float(mad)))
    bound = ms.sequence_chunk_sample_bound(spec["bases"], fp)
    assert bound == int(np.floor((spec["bases"] + 1e-8) * (med + spec["filter_mean_dwell"] * mad))) + 1
    assert all(int(x) <= bound for x in g["chunk_siglen"])
    assert ms.sequence_chunk_sample_bound(spec["bases"], ms.FILTER_PARAMETERS(**filter_dict(spec, on=False))) is None


def test_regions_of_reads_with_nothing_mapped():
    read = dict(Dacs=np.zeros(50, np.int16), Ref_to_signal=np.array([-1, -1, 51, 51], np.int32))
    assert list(ms.mapped_reference_regions([read])[0]) == [0, 0] == list(support.mapped_reference_region(read))
    read = dict(Dacs=np.zeros(50, np.int16), Ref_to_signal=np.array([-1, 3, 9, 50, 51], np.int32))
    assert list(ms.mapped_reference_regions([read])[0]) == [1, 3] == list(support.mapped_reference_region(read))


def _exported(libname):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                         capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_binding_and_exports_name_the_same_entries():
    assert set(_lib.CHUNKS_SEQLEN_SIGNATURES) == ENTRIES == _exported(_lib.CHUNKS_SEQLEN_LIBNAME)
    _lib.chunks_seqlen_lib()                            # resolves every symbol
    sz, i, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    assert _lib.CHUNKS_SEQLEN_SIGNATURES["tk_chunks_seqlen_locate_dev"] == (i, [vp] * 5 + [sz, sz] + [vp] * 7)
    assert _lib.CHUNKS_SEQLEN_SIGNATURES["tk_chunks_seqlen_gather_dev"] == (
        i, [vp] * 8 + [sz, sz, i, i, vp, vp, sz] + [vp] * 5)
    # the main library and its header are what they were
    assert not any("seqlen_" in name for name in _exported(_lib.LIBNAME))
    assert not any("chunks_seqlen" in name for name in _lib.SIGNATURES)
    assert _lib.DEFINES["TK_STATUS_SEQS_OVERFLOW"] == 4 and _lib.DEFINES["TK_CHUNK_NREASON"] == len(REASONS)


def test_entry_points_refuse_before_they_launch():
    L = _lib.chunks_seqlen_lib()
    bad, unsupported = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED"))
    p = ctypes.c_void_p(4096)
    store = ms._Store(4096, 4096, 4096, 4096, 4096, 4096, 4096, 3)
    filt = ms._Filter(0, 1, 0.0, 0.0, 0.0, 0.0, 0.0)
    table = (ctypes.c_float * 12)()
    s, f = ctypes.byref(store), ctypes.byref(filt)
    locate, gather = L.tk_chunks_seqlen_locate_dev, L.tk_chunks_seqlen_gather_dev
    assert locate(s, p, p, p, None, 0, 30, f, p, p, p, p, p, None) == 0              # no candidates: nothing to do
    assert locate(s, p, p, p, None, 8, 0, f, p, p, p, p, p, None) == bad             # chunk_bases 0
    assert locate(s, None, p, p, None, 8, 30, f, p, p, p, p, p, None) == bad         # no mapped_ref
    assert locate(s, p, p, None, None, 8, 30, f, p, p, p, p, p, None) == bad         # neither start nor fraction
    assert locate(None, p, p, p, None, 8, 30, f, p, p, p, p, p, None) == bad
    assert locate(s, p, p, p, None, 1 << 31, 30, f, p, p, p, p, p, None) == unsupported
    assert locate(s, p, p, p, None, 8, 1 << 31, f, p, p, p, p, p, None) == unsupported
    assert gather(s, p, p, p, p, p, p, p, 0, 30, 0, 1, table, p, 100, p, p, p, p, None) == 0      # nwant 0
    assert gather(s, p, p, p, p, p, p, p, 4, 0, 0, 1, table, p, 100, p, p, p, p, None) == bad     # chunk_bases 0
    assert gather(s, p, p, p, p, p, p, p, 4, 30, 0, 1, None, p, 100, p, p, p, p, None) == bad     # no table
    assert gather(s, p, p, p, p, p, p, p, 4, 30, 0, 1, table, None, 100, p, p, p, p, None) == bad
    assert gather(s, p, p, p, p, p, p, p, 1 << 31, 30, 0, 1, table, p, 100, p, p, p, p, None) == unsupported
    assert gather(s, p, p, p, p, p, p, p, 4, 30, 0, 1, table, p, 1 << 40, p, p, p, p, None) == unsupported


def test_python_refuses_a_chunk_without_bases():
    """(checked before any device is touched: the store here was never built)"""
    store = object.__new__(ms.MappedSignalStore)
    fp = ms.FILTER_PARAMETERS(3.0, 10.0, 0.5, None, None, None, None)
    for bases in (0, -3):
        with pytest.raises(ValueError, match="chunk_bases"):
            store.sample_sequence_chunks(4, bases, fp)
        with pytest.raises(ValueError, match="chunk_bases"):
            store.sample_chunks(4, bases, fp, chunk_len_means_sequence_len=True)
    with pytest.raises(ValueError, match="bases, not flip-flop codes"):
        store.sample_chunks(4, 30, fp, mod_labels=[0, 0, 0, 0, 1], can_labels=[0, 1, 2, 3, 1],
                            chunk_len_means_sequence_len=True)
    import torch
    reads = spec_reads(SPECS["r20b1"])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ms.MappedSignalStore(reads, torch.device("cpu"))
