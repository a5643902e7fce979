"""Beam-search basecalling of batches of reads on the device: tk_basecall_stitch_scores_dev, tk_basecall_beamsearch_dev
(include/taiyaki_amd_basecall.h, (d) and (e)), decodeutil.beamsearch_batch and Basecaller(beam=(width, guided)).

CPU: the ABI and the construction checks.  GPU: the stitch kernel against basecall_helpers.stitch_chunks bit for bit,
the variable-length search against the oracle restatement (correctly rounded exp / log1p, as the kernel's) and against
the dense entry point on every read alone, sequences and float scores bit for bit, and the whole call against the chain
of existing operators.  Every kernel is launched once per check."""
import ctypes
import json
import os
import re
import subprocess

import numpy as np
import pytest

from oracle import beam
from tests import basecall_support as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHUNK_PLAN = 256


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW"}


def test_abi_new_entry_points_are_in_the_basecall_library_only():
    from taiyaki_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "taiyaki_amd_basecall.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"^(?:const\s+)?[a-z_0-9]+\s+\*?\s*([a-z_0-9]+)\(", hdr, flags=re.M))
    new = {"tk_basecall_stitch_scores_dev", "tk_basecall_beamsearch_dev", "tk_basecall_beamsearch_workspace_bytes"}
    assert new <= declared
    assert _exported(os.path.join(_lib.CSRC, _lib.BASECALL_LIBNAME)) == declared == set(_lib.BASECALL_SIGNATURES)
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "abi_signatures.json")))
    assert len(golden["SIGNATURES"]) == 43 and _exported(_lib.LIBPATH) == set(golden["SIGNATURES"])
    L = _lib.basecall_lib()
    assert L.tk_basecall_version() == b"taiyaki_amd basecall gfx950 r2"
    # guiding matrix (rows + one per read) x 2 nbase floats, rounded to 256, + 16 back-pointer bytes per row + 512
    assert L.tk_basecall_beamsearch_workspace_bytes(1000, 3, 4) == (1003 * 8 * 4 + 255) // 256 * 256 + 16000 + 512
    assert L.tk_basecall_beamsearch_workspace_bytes(0, 0, 4) == 512


def test_basecaller_checks_its_beam_arguments_before_the_device():
    import torch
    from taiyaki_amd import basecall
    cpu_model = torch.nn.Linear(1, 1)
    bad = [dict(beam=(5, True), fastq=True), dict(beam=(0, True)), dict(beam=(13, True)), dict(beam=(2.5, True)),
           dict(beam=(5, True), beam_cut=-0.1), dict(beam=(5, True), beam_cut=1.5), dict(beam=(5, True), beam_cut=float("nan")),
           dict(beam=5), dict(beam=(12, True), alphabet="ACGTZ"), dict(beam=(5, True), alphabet="ACGTZ")]
    for kw in bad:
        with pytest.raises(ValueError):
            basecall.Basecaller(cpu_model, **kw)
        with pytest.raises(ValueError):
            basecall.check_beam(kw.get("beam"), kw.get("beam_cut", 0.0), len(kw.get("alphabet", "ACGT")), kw.get("fastq", False))
    # an admitted beam reaches the device check (this model is on the CPU), and so does no beam at all
    for kw in (dict(beam=(5, True)), dict(beam=(12, False), beam_cut=1.0), dict(beam=(1, True), beam_cut=0.0), dict()):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            basecall.Basecaller(cpu_model, **kw)
    assert basecall.check_beam(None, 7.0, 4, True) is None                  # no beam: nothing to check
    assert basecall.check_beam((5, 1), 0.0, 4, False) == basecall.Beam(5, True)
    assert basecall.check_beam((12, False), 1.0, 4, False) == (12, False)   # 12 * 5 = 60 records: the widest
    assert basecall.check_beam((12, True), 0.0, 3, False).width == 12


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the stitch kernel
# ----------------------------------------------------------------------------------------------------------------------
def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


# the chunk geometries of bs.TAILS, one with overlap 0, and one whose overlap (37 samples, stride 2) is odd: the cut
# between two chunks, 37 // 4, is decided by the floor division
GEOMETRIES = dict({k: {f: v[f] for f in ("T", "stride", "overlap", "N", "ragged")} for k, v in bs.TAILS.items()},
                  zero_overlap=dict(T=300, stride=5, overlap=0, N=3, ragged=203),
                  odd_overlap=dict(T=250, stride=2, overlap=37, N=4, ragged=5))
GROUPS = {(300, 5): ["one", "two", "twenty", "zero_overlap"], (250, 2): ["stride2", "odd_overlap"]}
FILL = 0x7fc12345                                                           # a NaN no score is


def _bounds(spec):
    from taiyaki_amd import basecall_helpers
    starts, ends = basecall_helpers.chunk_bounds(bs.tail_siglen(spec), spec["T"] * spec["stride"], spec["overlap"])
    assert len(starts) == spec["N"]
    return starts.astype(np.int64), ends.astype(np.int64)


def _stitch(trans, geos, stride, dev, room=None, scale=None, margin=7):
    """tk_basecall_stitch_scores_dev, one launch: `trans` (T, sum of chunks, S), geos = [(starts, ends)] per read ->
    (packed as uint32 (total, S), row_off, nrows, status)"""
    import torch
    from taiyaki_amd import _lib
    T, nch, S = trans.shape
    counts = [len(g[0]) for g in geos]
    assert sum(counts) == nch
    rco = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    if room is None:
        room = [T * n for n in counts]
    row_off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    total = int(row_off[-1])
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)  # noqa: E731
    d = [t(trans, np.float32), t(np.concatenate([g[0] for g in geos]), np.int64),
         t(np.concatenate([g[1] for g in geos]), np.int64), t(rco, np.int64), t(row_off, np.int64),
         t(scale, np.float32) if scale is not None else None]
    packed = torch.full((total + margin, S), FILL, dtype=torch.int32, device=dev)   # a margin past the last read
    nrows = torch.full((len(geos),), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    rc = _lib.basecall_lib().tk_basecall_stitch_scores_dev(
        _p(d[0]), T, nch, S, _p(d[1]), _p(d[2]), _p(d[3]), _p(d[5]), len(geos), stride, _p(d[4]), total, _p(packed),
        _p(nrows), _p(status), None)
    assert rc == 0, rc
    return packed.cpu().numpy().view(np.uint32), row_off, nrows.cpu().numpy(), int(status.item())


def _want_stitched(trans, geo, stride):
    import torch
    from taiyaki_amd import basecall_helpers
    return basecall_helpers.stitch_chunks(torch.from_numpy(trans), geo[0], geo[1], stride).numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("group", list(GROUPS))
def test_stitch_kernel_is_stitch_chunks_bit_for_bit(gpu_device, group):
    from taiyaki_amd import basecall
    (T, stride), names = group, GROUPS[group]
    geos = [_bounds(GEOMETRIES[n]) for n in names]
    nch = sum(len(g[0]) for g in geos)
    trans = (np.random.RandomState(T + stride).randn(T, nch, 40) * 3).astype(np.float32)
    cols = np.concatenate([[0], np.cumsum([len(g[0]) for g in geos])])
    packed, row_off, nrows, status = _stitch(trans, geos, stride, gpu_device)       # every read in ONE launch
    assert status == 0
    for i, n in enumerate(names):
        spec = GEOMETRIES[n]
        own = np.ascontiguousarray(trans[:, cols[i]:cols[i + 1]])
        want = _want_stitched(own, geos[i], stride)
        lo = int(row_off[i])
        assert nrows[i] == len(want) == basecall.stitched_rows(spec["N"], bs.tail_siglen(spec), T * stride,
                                                               spec["overlap"], stride, T), n
        assert packed[lo:lo + nrows[i]].tobytes() == want.tobytes(), n
        assert (packed[lo + nrows[i]:int(row_off[i + 1])] == FILL).all(), n         # rows past the count: untouched
        alone, off1, n1, s1 = _stitch(own, [geos[i]], stride, gpu_device)           # the read alone: the same bytes
        assert s1 == 0 and n1[0] == nrows[i] and alone[:n1[0]].tobytes() == want.tobytes(), n
        assert (alone[n1[0]:] == FILL).all(), n
        if spec["N"] == 1:
            assert nrows[i] == T                                                    # one chunk keeps all its rows
    assert (packed[int(row_off[-1]):] == FILL).all()
    # rooms of exactly the stitched row counts (what Basecaller gives), and a NaN read_scale: that read gets 0 rows
    room = [int(n) for n in nrows]
    scale = np.ones(len(names), dtype=np.float32)
    scale[1] = np.nan
    tight, off2, n2, s2 = _stitch(trans, geos, stride, gpu_device, room=room, scale=scale)
    assert s2 == 0 and n2[1] == 0 and list(np.delete(n2, 1)) == list(np.delete(nrows, 1))
    assert (tight[int(off2[1]):int(off2[2])] == FILL).all()
    for i in [k for k in range(len(names)) if k != 1]:
        assert tight[int(off2[i]):int(off2[i]) + n2[i]].tobytes() == packed[int(row_off[i]):int(row_off[i]) + nrows[i]].tobytes()


@pytest.mark.gpu
def test_stitch_kernel_reports_a_room_that_is_too_small(gpu_device):
    """The read that lacks room is the LAST one, and the buffer goes on for 128 rows past the `total_rows` the kernel is
    given: the 101 rows that do not fit would land there, where nothing else writes."""
    geos = [_bounds(GEOMETRIES[n]) for n in ("twenty", "two")]
    trans = (np.random.RandomState(3).randn(300, 22, 40)).astype(np.float32)
    full, off, nrows, status = _stitch(trans, geos, 5, gpu_device)
    assert status == 0
    room = [int(nrows[0]), int(nrows[1]) - 101]              # 101 rows short: the cut falls inside the read's chunk 2
    part, off2, n2, status = _stitch(trans, geos, 5, gpu_device, room=room, margin=128)
    assert status == CHUNK_PLAN and list(n2) == room
    assert part[:room[0]].tobytes() == full[:room[0]].tobytes()                     # the read before it: whole
    lo = int(off2[1])
    assert part[lo:lo + room[1]].tobytes() == full[int(off[1]):int(off[1]) + room[1]].tobytes()    # what fits is written
    assert len(part) == lo + room[1] + 128 and (part[lo + room[1]:] == FILL).all()  # ... and nothing beyond it


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the search for reads of different lengths
# ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def correctly_rounded_oracle():
    old, beam.MATH = beam.MATH, "cr"
    yield beam
    beam.MATH = old


def quantised_scores(T, seed, step=0.5):
    """Scores on a grid of `step`: different paths reach EXACTLY equal scores all the time, and the beam depends on the
    order the reference's quicksort leaves equal records in (ties in nearly every block)."""
    rng = np.random.RandomState(seed)
    return (np.round(rng.randn(T, 40) * 2 / step) * step).astype(np.float32)


LENGTHS = (0, 1, 2, 37, 64, 65, 180, 300)


def _packed_search(reads, dev, width, cut, guided, alphabet=b"ACGT", gap=3):
    """tk_basecall_beamsearch_dev, one launch, every read in a room `gap` rows longer than itself, outputs pre-filled
    -> per read (states, score, call), after checking that nothing was written past a read's counts."""
    import torch
    from taiyaki_amd import _lib, flipflopfings
    L = _lib.basecall_lib()
    S, nbase = reads[0].shape[1], len(alphabet)
    lens = np.array([len(r) for r in reads], dtype=np.int64)
    row_off = np.concatenate([[0], np.cumsum(lens + gap)]).astype(np.int64)
    total = int(row_off[-1])
    host = np.full((total, S), np.nan, dtype=np.float32)                            # the gaps hold NaN: never read
    for r, lo in zip(reads, row_off):
        host[lo:lo + len(r)] = r
    d_sc, d_off = torch.from_numpy(host).to(dev), torch.from_numpy(row_off).to(dev)
    d_n = torch.from_numpy(lens.astype(np.int32)).to(dev)
    states = torch.full((total,), 99, dtype=torch.int8, device=dev)
    seq = torch.full((total,), ord("."), dtype=torch.uint8, device=dev)
    nstate, seqlen = (torch.full((len(reads),), -7, dtype=torch.int32, device=dev) for _ in range(2))
    score = torch.full((len(reads),), -7.0, dtype=torch.float32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    wsb = L.tk_basecall_beamsearch_workspace_bytes(total, len(reads), nbase)
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    rc = L.tk_basecall_beamsearch_dev(_p(d_sc), _p(d_off), _p(d_n), len(reads), total, int(lens.max()) + gap, nbase,
                                      alphabet, width, cut, int(guided), _p(states), _p(nstate), _p(score), _p(seq),
                                      _p(seqlen), _p(ws), wsb, _p(status), None)
    assert rc == 0, rc
    states, seq, nstate, seqlen = states.cpu().numpy(), seq.cpu().numpy(), nstate.cpu().numpy(), seqlen.cpu().numpy()
    assert int(status.item()) == 0
    out = []
    for i, lo in enumerate(row_off[:-1]):
        hi = int(row_off[i + 1])
        st, call = states[lo:lo + nstate[i]], seq[lo:lo + seqlen[i]].tobytes().decode()
        assert 0 <= nstate[i] <= lens[i] and (states[lo + nstate[i]:hi] == 99).all()        # nothing past the counts
        assert (seq[lo + seqlen[i]:hi] == ord(".")).all()
        assert call == flipflopfings.path_to_str(st, alphabet=alphabet.decode(), include_first_source=False) if len(st) else call == ""
        out.append((st, score.cpu().numpy()[i], call))
    return out


def _check_against_both(reads, dev, oracle, width, cut, guided, alphabet=b"ACGT", with_oracle=True):
    import torch
    from taiyaki_amd import decodeutil
    got = _packed_search(reads, dev, width, cut, guided, alphabet)
    for r, (st, sc, call) in zip(reads, got):
        tag = (len(r), width, cut, guided)
        if len(r) == 0:
            assert len(st) == 0 and call == "" and sc.tobytes() == np.float32(0).tobytes(), tag     # the stated answer
            continue
        if with_oracle:
            ws, wsc = oracle.beamsearch(r, cut, width, guided)
            assert np.array_equal(st, ws) and sc.tobytes() == np.float32(wsc).tobytes(), tag
        ds, dsc = decodeutil.beamsearch(torch.from_numpy(r).to(dev), cut, width, guided)           # the read alone, N = 1
        assert st.dtype == ds.dtype == np.int8 and np.array_equal(st, ds), tag
        assert sc.tobytes() == np.float32(dsc).tobytes(), tag
    return got


@pytest.mark.gpu
def test_packed_beamsearch_continuous_scores(gpu_device, correctly_rounded_oracle):
    from taiyaki_amd import decodeutil, synth
    reads = [np.ascontiguousarray(synth.scores(T, 1, 40, 300 + T)[:, 0] * np.float32(0.8)) if T else
             np.zeros((0, 40), dtype=np.float32) for T in LENGTHS]
    got = _check_against_both(reads, gpu_device, correctly_rounded_oracle, 5, 0.0, True)
    assert sum(len(g[2]) for g in got) > 200 and [len(g[0]) for g in got[:2]] == [0, 1]
    # the public wrapper: the same launch, numpy arrays or device tensors in
    import torch
    mixed = [torch.from_numpy(r).to(gpu_device) if i % 2 else r for i, r in enumerate(reads)]
    seqs, scores = decodeutil.beamsearch_batch(mixed, 0.0, 5, True)
    assert scores.dtype == np.float32 and scores.shape == (len(reads),)
    for (st, sc, _), s2, sc2 in zip(got, seqs, scores):
        assert s2.dtype == np.int8 and np.array_equal(st, s2) and sc.tobytes() == sc2.tobytes()
    with pytest.raises(ValueError):
        decodeutil.beamsearch_batch(reads, 0.0, 13, True)
    with pytest.raises(ValueError):
        decodeutil.beamsearch_batch(reads, 1.5, 5, True)


@pytest.mark.gpu
@pytest.mark.parametrize("width,cut,guided", [(3, 0.0, True), (12, 0.0, True), (5, 0.05, True), (5, 0.0, False)])
def test_packed_beamsearch_through_exact_ties(gpu_device, correctly_rounded_oracle, width, cut, guided):
    reads = [quantised_scores(T, 700 + T) for T in LENGTHS]
    _check_against_both(reads, gpu_device, correctly_rounded_oracle, width, cut, guided)


@pytest.mark.gpu
@pytest.mark.parametrize("nbase", [1, 2, 3])
def test_packed_beamsearch_other_alphabets(gpu_device, correctly_rounded_oracle, nbase):
    rng = np.random.RandomState(60 + nbase)
    reads = [(rng.randn(T, 2 * nbase * (nbase + 1)) * 2).astype(np.float32) for T in (0, 1, 30, 65)]
    _check_against_both(reads, gpu_device, correctly_rounded_oracle, 4, 0.0, True, alphabet=b"ACG"[:nbase])


@pytest.mark.gpu
def test_packed_beamsearch_long_read_in_hbm_beside_a_short_one_in_lds(gpu_device):
    """3700 rows are more than the 3584 back-pointer rows the LDS window holds: that read walks back through HBM while
    the 50-row read of the same launch sits in the window.  Against the dense entry point only."""
    from taiyaki_amd import synth
    reads = [np.ascontiguousarray(synth.scores(T, 1, 40, 91 + T)[:, 0] * np.float32(0.8)) for T in (3700, 50)]
    got = _check_against_both(reads, gpu_device, None, 5, 0.0, True, with_oracle=False)
    assert len(got[0][0]) > 1000


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the whole call
# ----------------------------------------------------------------------------------------------------------------------
READS = ("len1", "len2", "len4999", "len5000", "len5001", "len9500", "len23456", "constant")


def _model(which, dev):
    import torch
    from taiyaki_amd import models, synth
    if which == "gru":
        torch.manual_seed(13)
        net, stride = models.mGru_flipflop(size=96, stride=2), 2
    else:
        torch.manual_seed(14)
        net, stride = models.mLstm_flipflop(size=64, stride=5), 5
    return synth.excite_network(net.to(dev).eval()), stride


def _beam_chain(x, model, stride, dev, posterior, temperature, width, guided, cut=0.0, concurrent=16):
    """bin/basecall.py:151-221 with a beam on this package's existing operators and host helpers, one read."""
    import torch
    from taiyaki_amd import basecall_helpers, clipping, decode, decodeutil, flipflopfings
    med, mad = clipping.med_mad(x)
    if not mad > 0:
        return "", None, len(x)
    normed = ((x - med) / mad).astype("f4")
    chunks, starts, ends = basecall_helpers.chunk_read(normed, bs.CHUNK_BLOCKS * stride, bs.OVERLAP_BLOCKS * stride)
    with torch.no_grad():
        chunks = torch.tensor(chunks, device=dev)
        trans = torch.cat([model(c.contiguous())[:, :, :40] for c in torch.split(chunks, concurrent, 1)], 1) * temperature
        if posterior:
            trans = (decode.flipflop_make_trans(trans) + 1e-8).log()
        stitched = basecall_helpers.stitch_chunks(trans, starts, ends, stride)
        best, _ = decodeutil.beamsearch(stitched.contiguous(), cut, width, guided)
    return flipflopfings.path_to_str(best, alphabet="ACGT", include_first_source=False), None, len(x)


@pytest.mark.gpu
@pytest.mark.parametrize("temperature", [1.0, 0.7])
@pytest.mark.parametrize("posterior", [True, False])
@pytest.mark.parametrize("which", ["gru", "lstm"])
def test_beam_basecaller_equals_the_chain_of_existing_operators(gpu_device, which, posterior, temperature):
    from taiyaki_amd import basecall
    model, stride = _model(which, gpu_device)
    caller = basecall.Basecaller(model, chunk_size=bs.CHUNK_BLOCKS, overlap=bs.OVERLAP_BLOCKS, max_concurrent_chunks=16,
                                 posterior=posterior, temperature=temperature, pack=False, beam=(5, True))
    assert caller.stride == stride
    sigs, alone = [bs.signal(n) for n in READS], []
    for n, x in zip(READS, sigs):                                   # one read per call
        got, = caller.call([x])
        want = _beam_chain(x, model, stride, gpu_device, posterior, temperature, 5, True)
        assert got == want and got[2] == len(x) and got[1] is None, (which, n, posterior, temperature)
        if n in ("len1", "constant"):
            assert got[0] == ""
        alone.append(got)
    print(which, "posterior", posterior, "temperature", temperature, "bases called:", [len(r[0]) for r in alone])
    assert sum(len(r[0]) for r in alone) > 1000                     # (the comparison is not one of empty strings)
    assert caller.call(sigs) == alone                               # the same reads as ONE batch: one beam launch
    # a short read and a read without samples BETWEEN reads of several chunks (the chain calls nothing without samples)
    empty = np.zeros(0, dtype=np.float32)
    assert _beam_chain(empty, model, stride, gpu_device, posterior, temperature, 5, True) == ("", None, 0)
    order = ("len9500", "len4999", None, "len23456", "len2", "len5001")
    want = [alone[READS.index(n)] if n else ("", None, 0) for n in order]
    assert caller.call([sigs[READS.index(n)] if n else empty for n in order]) == want
    assert all(len(want[i][0]) > 0 for i in (0, 1, 3, 5))           # (not a comparison of empty calls)


@pytest.mark.gpu
def test_beam_basecaller_unguided_and_no_beam(gpu_device):
    from taiyaki_amd import basecall
    model, stride = _model("lstm", gpu_device)
    kw = dict(chunk_size=bs.CHUNK_BLOCKS, overlap=bs.OVERLAP_BLOCKS, max_concurrent_chunks=16, pack=False)
    x = bs.signal("len9500")
    got, = basecall.Basecaller(model, beam=(3, False), beam_cut=0.05, **kw).call([x])
    assert got == _beam_chain(x, model, stride, gpu_device, True, 1.0, 3, False, cut=0.05) and len(got[0]) > 100
    # beam=None is the Viterbi call of a Basecaller constructed without the argument
    sigs = [bs.signal(n) for n in ("len2", "len4999", "len9500", "constant")]
    for fastq in (False, True):
        assert basecall.Basecaller(model, beam=None, fastq=fastq, **kw).call(sigs) == \
            basecall.Basecaller(model, fastq=fastq, **kw).call(sigs)
