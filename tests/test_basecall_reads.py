"""Basecalling batches of reads on the device (include/taiyaki_amd_basecall.h, taiyaki_amd/basecall.py).

Fixtures: tests/golden/basecall_reads.npz, written by the genuine reference (make_golden_basecall_reads.py) on the
seeded signals and tail cases of tests/basecall_support.py.  The tail cases keep every error probability inside
(1e-9, 1) and every overlap > 0, so the reference never meets e <= 0 there (the generator asserts it); the two places
where the kernels depart from the reference (e == 0, e < 0) are asserted against the header's stated behaviour.

CPU: the ABI, chunk_read, the numpy restatement of the tail, the packing plan.  GPU: the three kernels, the whole
call against the chain of existing operators, and packing as a pure regrouping."""
import itertools
import os
import re
import subprocess

import numpy as np
import pytest

from tests import basecall_support as bs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def _exported(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW"}


def test_basecall_abi_is_the_header():
    from taiyaki_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "taiyaki_amd_basecall.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"^(?:const\s+)?[a-z_0-9]+\s+\*?\s*([a-z_0-9]+)\(", hdr, flags=re.M))
    assert {"tk_signal_med_mad_dev", "tk_basecall_gather_chunks_dev", "tk_basecall_call_dev"} <= declared
    new = _exported(os.path.join(_lib.CSRC, _lib.BASECALL_LIBNAME))
    assert new == declared
    assert set(_lib.BASECALL_SIGNATURES) == declared
    assert not new & _exported(_lib.LIBPATH)                    # the pinned library gained nothing
    assert not set(_lib.BASECALL_SIGNATURES) & (set(_lib.SIGNATURES) | set(_lib.RCCL_SIGNATURES))
    L = _lib.basecall_lib()                                      # resolves every symbol
    assert L.tk_basecall_version().startswith(b"taiyaki_amd basecall")
    # the chunk count's closed form is chunk_read's count
    from taiyaki_amd import basecall, basecall_helpers
    for n in (1, 4999, 5000, 5001, 9499, 9500, 9501, 14000, 14001, 100003):
        want = len(basecall_helpers.chunk_bounds(n, bs.CHUNK, bs.OVERLAP)[0]) if n >= bs.CHUNK else 0
        assert L.tk_basecall_chunk_count(n, bs.CHUNK, bs.OVERLAP) == want == basecall.chunk_counts([n], bs.CHUNK, bs.OVERLAP)[0]


@pytest.mark.parametrize("name", list(bs.SIGNALS))
def test_chunk_read_matches_reference(name):
    from taiyaki_amd import basecall_helpers, clipping
    g, x = bs.load(), bs.signal(name)
    med, mad = clipping.med_mad(x)
    assert np.float32(med).tobytes() == g[name + "/med"].tobytes() and np.float32(mad).tobytes() == g[name + "/mad"].tobytes()
    normed = ((x - med) / mad).astype("f4") if mad > 0 else x
    chunks, starts, ends = basecall_helpers.chunk_read(normed, bs.CHUNK, bs.OVERLAP)
    np.testing.assert_array_equal(starts, g[name + "/chunk_starts"])
    np.testing.assert_array_equal(ends, g[name + "/chunk_ends"])
    assert chunks.shape == tuple(g[name + "/chunks_shape"]) and chunks.dtype == np.float32
    if len(x) < bs.CHUNK:
        assert chunks.shape == (len(x), 1, 1)
    assert bs.crc(chunks) == int(g[name + "/chunks_crc"])
    np.testing.assert_array_equal(chunks[:, 0, 0], g[name + "/first_chunk"])
    np.testing.assert_array_equal(chunks[:, -1, 0], g[name + "/last_chunk"])


@pytest.mark.parametrize("name", list(bs.TAILS))
def test_numpy_tail_restatement_matches_reference(name):
    """numpy doing numpy's arithmetic: sequences AND quality strings exact, no tolerance."""
    g, spec, p = bs.load(), bs.TAILS[name], "tail/%s/" % name
    path, err = g[p + "path"].astype(np.int64), g[p + "errprobs"]
    for tag, (scale, offset) in bs.QSETTINGS.items():
        seq, q, sp = bs.tail(path, err, g[p + "chunk_starts"], g[p + "chunk_ends"], spec["stride"], "ACGT", scale, offset)
        np.testing.assert_array_equal(sp, g[p + "stitched_path"])
        assert seq == bytes(g[p + "seq"]).decode() and q == bytes(g[p + tag]).decode()
    assert bs.tail(path, None, g[p + "chunk_starts"], g[p + "chunk_ends"], spec["stride"])[1] is None
    from taiyaki_amd import basecall
    assert basecall.stitched_rows(spec["N"], bs.tail_siglen(spec), spec["T"] * spec["stride"], spec["overlap"],
                                  spec["stride"], path.shape[0]) == len(g[p + "stitched_path"])


@pytest.mark.parametrize("pack", [True, False])
@pytest.mark.parametrize("width", [1, 3, 16, 128])
def test_packing_plan(pack, width):
    from taiyaki_amd import basecall
    lengths = [n for n, _, _ in bs.SIGNALS.values()] + [0, 5000, 50000]
    counts = basecall.chunk_counts(lengths, bs.CHUNK, bs.OVERLAP)
    plan = basecall.packing_plan(lengths, bs.CHUNK, bs.OVERLAP, width, pack)
    long_slices, short_slices = [s for s in plan if not s.short], [s for s in plan if s.short]
    # every chunk once, in read order: the slices tile [0, total) and the owners are the reads repeated by their counts
    assert [s.first for s in long_slices] == list(np.cumsum([0] + [s.ncol for s in long_slices])[:-1])
    owners = list(itertools.chain.from_iterable(s.reads for s in long_slices))
    assert owners == list(np.repeat(np.arange(len(lengths)), counts))
    assert all(0 < s.ncol <= width and len(s.reads) == s.ncol for s in plan)
    if not pack:
        assert all(len(set(s.reads)) == 1 for s in long_slices)
    else:
        assert all(s.ncol == width for s in long_slices[:-1])           # full slices, across read boundaries
    # short reads: one column each, in read order; a read without samples is not run
    assert [s.first for s in short_slices] == [r for r, n in enumerate(lengths) if 0 < n < bs.CHUNK]
    assert all(s.ncol == 1 and s.reads == (s.first,) for s in short_slices)


def test_transfer_layouts_and_room_of_a_hand_written_batch():
    """Three reads of 9500, 3 and 5002 samples at stride 5 (two chunks, a short read between, two chunks): the byte
    layouts of the upload and of the download, and every read's room, as literals worked out by hand from 16-byte
    alignment and the stitching cuts (9500: rows [0, 950) + [50, 1000); 5002: [0, 500) + [499, 1000); 3: its own 2)."""
    from taiyaki_amd import basecall
    offsets = lambda lay: {k: v[0] for k, v in lay.fields.items()}  # noqa: E731
    up = basecall._Layout([("signal", np.float32, 14505), ("sig_off", np.int64, 4), ("shift", np.float32, 3),
                           ("scale", np.float32, 3)])
    assert offsets(up) == dict(signal=0, sig_off=58032, shift=58064, scale=58080)
    assert up.nbytes == 58092 and basecall._align(up.nbytes) == 58096
    head = basecall._Layout([("seqlen", np.int32, 3), ("status", np.uint8, 16)])
    assert offsets(head) == dict(seqlen=0, status=16) and head.nbytes == 32
    counts = basecall.chunk_counts([9500, 3, 5002], bs.CHUNK, bs.OVERLAP)
    assert counts.tolist() == [2, 0, 2]
    off = basecall.room_offsets(counts, [9500, 3, 5002], 1001, [(1, 2)], bs.CHUNK, bs.OVERLAP, bs.STRIDE)
    assert off.dtype == np.int64 and off.tolist() == [0, 1900, 1902, 2903]
    for nmod, nbytes in ((0, 5824), (2, 29048)):
        body = basecall._Layout([("seq", np.uint8, 2903), ("qual", np.uint8, 2903), ("mods", np.float32, 2903 * nmod)])
        assert offsets(body) == dict(seq=0, qual=2912, mods=5824) and body.nbytes == nbytes
    assert basecall._Layout([("seq", np.uint8, 2903)]).nbytes == 2903                  # a beam's download
    # typed views of a host block and, by the same names, of a tensor; `count` overrides the field's length
    import torch
    host = np.arange(up.nbytes, dtype=np.uint8)
    sig_off = up.view(host, "sig_off")
    assert sig_off.dtype == np.int64 and sig_off.shape == (4,) and sig_off.base is not None
    assert sig_off.tobytes() == host[58032:58064].tobytes() and up.view(host, "scale").tobytes() == host[58080:].tobytes()
    dev = torch.from_numpy(host)
    assert up.view(dev, "shift").dtype == torch.float32 and up.view(dev, "shift").numpy().tobytes() == host[58064:58076].tobytes()
    assert up.view(dev, "signal", 1).shape == (1,) and up.view(dev, "sig_off").data_ptr() == dev.data_ptr() + 58032
    # no read of a chunk or more: only the short ones have room
    assert basecall.room_offsets(np.zeros(3, dtype=np.int64), [0, 3, 7], 0, [(1, 2), (2, 3)], bs.CHUNK, bs.OVERLAP,
                                 bs.STRIDE).tolist() == [0, 0, 2, 5]


def test_write_records():
    import io
    from taiyaki_amd import basecall
    fh = io.StringIO()
    res = [("ACGT", "!!#~", 10), ("", "", 5), ("GG", "ab", 7)]
    assert basecall.write_records(fh, ["r1", "r2", "r3"], res, True) == (6, 2, 3, 22)
    assert fh.getvalue() == "@r1\nACGT\n+\n!!#~\n@r3\nGG\n+\nab\n"
    fh = io.StringIO()
    basecall.write_records(fh, ["r1"], [("ACGT", None, 10)], False, reverse=True)
    assert fh.getvalue() == ">r1\nTGCA\n"


def test_shim_exposes_the_chunk_helpers():
    from taiyaki_amd import basecall_helpers, shim
    shim.install(force_standalone=True)
    try:
        from taiyaki import basecall_helpers as tb
        assert tb.chunk_read is basecall_helpers.chunk_read and tb.run_model is basecall_helpers.run_model
    finally:
        shim.uninstall()


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the kernels at the C ABI.  Every kernel is launched once per check; nothing loops on a failing launch.
# ----------------------------------------------------------------------------------------------------------------------
# (the launches live in tests/basecall_support.py, which tests/test_basecall_glue_edges.py shares)
_p, _ok, _med_mad, _gather, _call = bs.dev_ptr, bs.ok, bs.med_mad_dev, bs.gather_dev, bs.call_dev
BAD_SIGNAL, CHUNK_PLAN = bs.BAD_SIGNAL, bs.CHUNK_PLAN


@pytest.mark.gpu
def test_med_mad_kernel_is_bit_equal_to_the_reference(gpu_device):
    g, names = bs.load(), list(bs.SIGNALS)
    sigs = [bs.signal(n) for n in names]
    med, mad, status = _med_mad(sigs, gpu_device)              # the whole batch in one launch
    assert status == BAD_SIGNAL                                 # len1 and constant: MAD == 0
    for i, n in enumerate(names):
        if g[n + "/mad"] > 0:
            assert med[i].tobytes() == g[n + "/med"].tobytes(), (n, med[i], g[n + "/med"])
            assert mad[i].tobytes() == g[n + "/mad"].tobytes(), (n, mad[i], g[n + "/mad"])
        else:
            assert n in ("len1", "constant") and np.isnan(med[i]) and np.isnan(mad[i])
    # one by one: bit for bit what the batch gave
    for i, n in enumerate(names):
        m1, d1, s1 = _med_mad([sigs[i]], gpu_device)
        assert m1.tobytes() == med[i:i + 1].tobytes() and d1.tobytes() == mad[i:i + 1].tobytes(), n
        assert s1 == (0 if g[n + "/mad"] > 0 else BAD_SIGNAL)
    # an injected NaN / inf: flagged, NaN out, the neighbours untouched
    for poison in (np.nan, np.inf):
        bad = bs.signal("len9500").copy()
        bad[1234] = poison
        m, d, s = _med_mad([sigs[4], bad, sigs[5]], gpu_device)
        assert s == BAD_SIGNAL and np.isnan(m[1]) and np.isnan(d[1])
        assert m[0] == med[4] and d[2] == mad[5]


@pytest.mark.gpu
@pytest.mark.parametrize("params", ["fixture", "caller"])
def test_gather_kernel_is_bit_equal_to_numpy(gpu_device, params):
    from taiyaki_amd import basecall_helpers
    g, names = bs.load(), [n for n in bs.SIGNALS if n not in ("len1", "constant")]
    sigs = [bs.signal(n) for n in names]
    if params == "fixture":
        shift, scale = [g[n + "/med"] for n in names], [g[n + "/mad"] for n in names]
    else:                                                        # the reference's --scaling path
        shift = [np.float32(88.5 + i) for i in range(len(names))]
        scale = [np.float32(9.75 + 0.5 * i) for i in range(len(names))]
    chunks, starts, ends, rco, status = _gather(sigs, shift, scale, gpu_device)
    assert status == 0
    at = 0
    for i, n in enumerate(names):
        assert rco[i] == at
        x = sigs[i]
        if len(x) < bs.CHUNK:
            continue                                             # called alone, below
        want, ws, we = basecall_helpers.chunk_read(((x - shift[i]) / scale[i]).astype("f4"), bs.CHUNK, bs.OVERLAP)
        k = want.shape[1]
        np.testing.assert_array_equal(starts[at:at + k], ws)
        np.testing.assert_array_equal(ends[at:at + k], we)
        assert chunks[:, at:at + k].tobytes() == want.tobytes(), n
        if params == "fixture":
            np.testing.assert_array_equal(ws, g[n + "/chunk_starts"])
            assert bs.crc(chunks[:, at:at + k]) == int(g[n + "/chunks_crc"]), n
        at += k
    assert rco[-1] == at == chunks.shape[1]
    # a short read is one chunk of its own length: the same kernel at chunk_size = len
    i = names.index("len4999")
    own, s1, e1, r1, st = _gather([sigs[i]], [shift[i]], [scale[i]], gpu_device, chunk=4999, overlap=0)
    assert st == 0 and own.shape == (4999, 1, 1) and (s1[0], e1[0], list(r1)) == (0, 4999, [0, 1])
    assert own.tobytes() == ((sigs[i] - shift[i]) / scale[i]).astype("f4").tobytes()
    if params == "fixture":
        assert bs.crc(own) == int(g["len4999/chunks_crc"])
    # a read that (a) refused (NaN shift / scale) becomes zeros
    z = _gather([sigs[names.index("len9500")]], [np.nan], [np.nan], gpu_device)
    assert z[4] == 0 and not z[0].any()


def _tail_case(g, name):
    p = "tail/%s/" % name
    return g[p + "path"].astype(np.int64), g[p + "errprobs"], g[p + "chunk_starts"], g[p + "chunk_ends"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(bs.TAILS))
def test_call_kernel_matches_reference(gpu_device, name):
    g, spec, p = bs.load(), bs.TAILS[name], "tail/%s/" % name
    path, err, starts, ends = _tail_case(g, name)
    want_seq = bytes(g[p + "seq"]).decode()
    for tag, (scale, offset) in bs.QSETTINGS.items():
        (seq, q), = _call(path, err, starts, ends, [0, spec["N"]], spec["stride"], gpu_device, scale, offset)
        want_q = bytes(g[p + tag]).decode()
        ndiff = sum(a != b for a, b in zip(q, want_q))
        print("%s %s: %d bases, %d quality characters differ from the reference" % (name, tag, len(seq), ndiff))
        assert seq == want_seq                                          # sequences and seqlen: exact
        assert bs.qstrings_close(q, want_q)
    (seq, q), = _call(path, None, starts, ends, [0, spec["N"]], spec["stride"], gpu_device)
    assert seq == want_seq and q is None


@pytest.mark.gpu
def test_call_kernel_batch_equals_per_read_launches(gpu_device):
    """Reads of 1, 2 and 20 chunks in one launch == one launch each."""
    g = bs.load()
    cases = [_tail_case(g, n) for n in ("one", "two", "twenty")]
    path, err = (np.concatenate([c[i] for c in cases], axis=1) for i in (0, 1))
    starts, ends = (np.concatenate([c[i] for c in cases]) for i in (2, 3))
    together = _call(path, err, starts, ends, [0, 1, 3, 23], 5, gpu_device, 0.9, 0.3)
    for (c, n), got in zip(zip(cases, (1, 2, 20)), together):
        assert _call(c[0], c[1], c[2], c[3], [0, n], 5, gpu_device, 0.9, 0.3) == [got]
    for name, got in zip(("one", "two", "twenty"), together):
        assert got[0] == bytes(g["tail/%s/seq" % name]).decode()


@pytest.mark.gpu
def test_call_kernel_clamps_where_the_reference_has_no_answer(gpu_device):
    """The header's two departures: e == 0 -> '~' (the reference converts +inf to int8), e < 0 -> NaN -> '!'; and the
    ends of the range, 126 and 33."""
    path = np.array([[0], [1], [2], [2], [3], [0], [5]], dtype=np.int64)          # moves at rows 1, 2, 4, 5, 6
    err = np.array([[-1], [0.0], [-1.0], [0.5], [1e-30], [1.0], [0.1]], dtype=np.float32)
    (seq, q), = _call(path, err, [0], [30], [0, 1], 5, gpu_device)
    assert seq == "CGTAC" and q == "~!~!+"                                         # -10 log10(0.1) = 10 -> '+'
    # room smaller than the call: reported through the status word, nothing written past it
    import torch
    from taiyaki_amd import _lib
    t = lambda a, dt: torch.from_numpy(np.asarray(a, dtype=dt)).to(gpu_device)  # noqa: E731
    buf = [t(path, np.int64), t([0], np.int64), t([30], np.int64), t([0, 1], np.int64), t([0, 3], np.int64)]
    seq_d = torch.full((8,), ord("."), dtype=torch.uint8, device=gpu_device)
    seqlen, status = torch.zeros(1, dtype=torch.int32, device=gpu_device), torch.zeros(1, dtype=torch.int32, device=gpu_device)
    _ok(_lib.basecall_lib().tk_basecall_call_dev(_p(buf[0]), None, 6, 1, _p(buf[1]), _p(buf[2]), _p(buf[3]), None, 1, 5, 4, b"ACGT",
                                                 1.0, 0.0, _p(buf[4]), _p(seq_d), None, _p(seqlen), _p(status), None))
    assert seq_d.cpu().numpy().tobytes() == b"CGT....." and int(seqlen.item()) == 3 and int(status.item()) == CHUNK_PLAN


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the whole call
# ----------------------------------------------------------------------------------------------------------------------
def _models(dev):
    import torch
    from taiyaki_amd import models
    torch.manual_seed(13)
    gru = models.mGru_flipflop(size=96, stride=2).to(dev).eval()
    torch.manual_seed(14)
    lstm = models.mLstm_flipflop(size=64, stride=5).to(dev).eval()
    # as initialised the stacks call no base at all, and the comparison below would be one of empty strings
    from taiyaki_amd import synth
    synth.excite_network(gru)
    synth.excite_network(lstm)
    return {"gru": (gru, 2), "lstm": (lstm, 5)}


def _qstring_where_defined(err, best, qs, qo):
    """qscores.path_errprobs_to_qstring, with the header's stated character where the reference has no answer inside
    '!' .. '~'.  With posterior off the "transition weights" handed to errprobs_from_trans are raw scores, so error
    probabilities fall outside (0, 1]: e <= 0 makes the reference convert NaN or +inf to int8 (undefined), e > 1 gives a
    code below '!'.  There the kernel's documented departures hold ('!' for NaN and below 33, '~' above 126) and are what
    is expected; every other character is the reference helper's own."""
    from taiyaki_amd import qscores
    picked = err[1:][best[1:] != best[:-1]].astype(np.float32)
    with np.errstate(invalid="ignore", divide="ignore"):
        code = (qs * qscores.qscore_from_errprob(picked) + qo) + 33 + 0.5
    low, high = ~(code >= 33), code >= 127                     # (NaN counts as low)
    fine = ~(low | high)
    stand_in = np.where(fine, picked, np.float32(0.5))
    q = np.frombuffer(qscores.qchar_from_errprob(stand_in, qs, qo).encode("ascii"), dtype=np.uint8).copy()
    q[low], q[high] = 33, 126
    return q.tobytes().decode("ascii")


def _reference_chain(x, model, stride, dev, posterior, temperature, fastq, qs, qo, width):
    """bin/basecall.py:151-242 on this package's existing operators and host helpers, one read."""
    import torch
    from taiyaki_amd import basecall_helpers, clipping, decode, flipflopfings, qscores
    med, mad = clipping.med_mad(x)
    if not mad > 0:
        return "", ("" if fastq else None), len(x)
    normed = ((x - med) / mad).astype("f4")
    chunks, starts, ends = basecall_helpers.chunk_read(normed, bs.CHUNK_BLOCKS * stride, bs.OVERLAP_BLOCKS * stride)
    with torch.no_grad():
        chunks = torch.tensor(chunks, device=dev)
        trans = torch.cat([model(c.contiguous())[:, :, :40] for c in torch.split(chunks, width, 1)], 1) * temperature
        if posterior:
            trans = (decode.flipflop_make_trans(trans) + 1e-8).log()
        _, _, cpath = decode.flipflop_viterbi(trans)
        best = basecall_helpers.stitch_chunks(cpath, starts, ends, stride).cpu().numpy()
        q = None
        if fastq:
            err = basecall_helpers.stitch_chunks(qscores.errprobs_from_trans(trans, cpath), starts, ends, stride)
            q = _qstring_where_defined(err.cpu().numpy(), best, qs, qo)
    return flipflopfings.path_to_str(best, alphabet="ACGT", include_first_source=False), q, len(x)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["gru", "lstm"])
def test_basecaller_equals_the_chain_of_existing_operators(gpu_device, which):
    """Real layers, ONE READ PER call with pack=False: every model invocation has the shape the reference's loop gives."""
    from taiyaki_amd import basecall
    model, stride = _models(gpu_device)[which]
    sigs = {n: bs.signal(n) for n in bs.SIGNALS}
    for posterior, temperature, fastq in itertools.product((True, False), (1.0, 0.7), (True, False)):
        caller = basecall.Basecaller(model, chunk_size=bs.CHUNK_BLOCKS, overlap=bs.OVERLAP_BLOCKS, max_concurrent_chunks=16,
                                     posterior=posterior, temperature=temperature, fastq=fastq, qscore_scale=0.9,
                                     qscore_offset=0.3, pack=False)
        assert caller.stride == stride
        called, alone = {}, {}
        for n, x in sigs.items():
            alone[n], = caller.call([x])
            seq, q, nsample = alone[n]
            wseq, wq, wn = _reference_chain(x, model, stride, gpu_device, posterior, temperature, fastq, 0.9, 0.3, 16)
            tag = (which, n, posterior, temperature, fastq)
            assert nsample == wn == len(x) and seq == wseq, tag
            if fastq:
                assert len(q) == len(seq) and bs.qstrings_close(q, wq), tag
            else:
                assert q is None and wq is None, tag
            if n in ("len1", "constant"):
                assert seq == ""
            called[n] = len(seq)
        print(which, "posterior", posterior, "temperature", temperature, "fastq", fastq, "bases called:", called)
        assert sum(called.values()) > 1000                          # (the comparison is not one of empty strings)
        # ONE batch with a short read and a read without samples between reads of several chunks: every read's call is
        # the one it got alone, above, where it was held against the chain (which calls nothing without samples)
        empty = np.zeros(0, dtype=np.float32)
        assert _reference_chain(empty, model, stride, gpu_device, posterior, temperature, fastq, 0.9, 0.3, 16) == \
            ("", "" if fastq else None, 0)
        batch = caller.call([sigs["len9500"], sigs["len4999"], empty, sigs["len23456"], sigs["len2"], sigs["len5001"]])
        assert batch == [alone["len9500"], alone["len4999"], ("", "" if fastq else None, 0), alone["len23456"],
                         alone["len2"], alone["len5001"]]
        assert all(len(batch[i][0]) > 0 for i in (0, 1, 3, 5))      # (the equality above is not one of empty calls)


@pytest.mark.gpu
def test_packing_is_only_a_regrouping(gpu_device):
    from taiyaki_amd import basecall
    net = bs.columnwise(gpu_device)
    names = list(bs.SIGNALS)
    sigs = [bs.signal(n) for n in names]
    kw = dict(stride=5, chunk_size=bs.CHUNK_BLOCKS, overlap=bs.OVERLAP_BLOCKS, max_concurrent_chunks=16, fastq=True)
    packed = basecall.Basecaller(net, pack=True, **kw).call(sigs)
    alone = basecall.Basecaller(net, pack=False, **kw)
    assert len(packed) == len(sigs)
    for n, x, got in zip(names, sigs, packed):
        assert alone.call([x]) == [got], n
        assert got[2] == len(x) and len(got[1]) == len(got[0])
    assert sum(len(r[0]) > 0 for r in packed) >= len(sigs) - 2
    # the caller's own shift / scale for some reads, median / MAD for the others, in one batch
    params = [(88.0, 11.5) if i % 2 else None for i in range(len(sigs))]
    mixed = basecall.Basecaller(net, pack=True, **kw).call(sigs, params)
    for i, (x, got) in enumerate(zip(sigs, mixed)):
        if params[i] is None:
            assert got == packed[i]
        else:
            assert got == alone.call([x], [params[i]])[0]
    # reversed signals are the reversed arrays called forwards
    rev = basecall.Basecaller(net, pack=True, reverse=True, **kw).call(sigs[3:6])
    assert rev == basecall.Basecaller(net, pack=True, **kw).call([s[::-1].copy() for s in sigs[3:6]])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["gru", "lstm"])
def test_packed_calls_with_real_layers_are_well_formed(gpu_device, which):
    """GEMMs may round differently at another column count, so packed calls of real models are only required to be
    well-formed records; how many equal the unpacked call is printed."""
    from taiyaki_amd import basecall
    model, _ = _models(gpu_device)[which]
    sigs = [bs.signal(n) for n in bs.SIGNALS]
    kw = dict(chunk_size=bs.CHUNK_BLOCKS, overlap=bs.OVERLAP_BLOCKS, max_concurrent_chunks=16, fastq=True)
    packed = basecall.Basecaller(model, pack=True, **kw).call(sigs)
    assert len(packed) == len(sigs)
    for x, (seq, q, n) in zip(sigs, packed):
        assert n == len(x) and len(q) == len(seq) and set(seq) <= set("ACGT")
        assert all(33 <= ord(c) <= 126 for c in q)
    unpacked = basecall.Basecaller(model, pack=False, **kw).call(sigs)
    same = sum(a[0] == b[0] for a, b in zip(packed, unpacked))
    print("%s: %d of %d reads have the same sequence packed and unpacked" % (which, same, len(sigs)))
