"""`Basecaller(batch_short=True)`: the reads shorter than a chunk called as zero-padded columns of shared tensors.

CPU: the packing plan.  GPU: the expected calls do not come from the code under test -- `layers.forward_varlen` on
columns normalised and padded in numpy, every column cut to its length, the existing fixed-length Viterbi on it (with
`posterior`: on the log of the new posterior operator's own column, which tests/test_decode_varlen.py holds against
float64), and the numpy restatement of the tail (tests/basecall_support.py)."""
import itertools

import numpy as np
import pytest

from tests import basecall_support as bs
from tests import mods_support as ms


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def test_packing_plan_groups_the_short_reads():
    from taiyaki_amd import basecall
    lengths = [9500, 3, 0, 5002, 4999, 1, 4998]
    today = basecall.packing_plan(lengths, 5000, 500, 2)
    assert basecall.packing_plan(lengths, 5000, 500, 2, batch_short=False) == today
    assert basecall.packing_plan(lengths, 5000, 500, 2, True, False) == today
    assert [s for s in today if s.short] == [basecall.Slice(True, r, 1, (r,)) for r in (1, 4, 5, 6)]
    plan = basecall.packing_plan(lengths, 5000, 500, 2, batch_short=True)
    assert [s for s in plan if not s.short] == [s for s in today if not s.short]
    assert [s for s in plan if s.short] == [basecall.Slice(True, 1, 2, (1, 4)), basecall.Slice(True, 5, 2, (5, 6))]
    assert not any(2 in s.reads for s in plan)                  # a read without samples is in none
    # a last slice that is not full; one wide enough for all; pack=False changes the long slices only
    assert [s.reads for s in basecall.packing_plan(lengths, 5000, 500, 3, batch_short=True) if s.short] == [(1, 4, 5), (6,)]
    assert [s.reads for s in basecall.packing_plan(lengths, 5000, 500, 128, batch_short=True) if s.short] == [(1, 4, 5, 6)]
    assert [s for s in basecall.packing_plan(lengths, 5000, 500, 2, False, True) if s.short] == [s for s in plan if s.short]
    assert basecall.packing_plan([0, 0], 5000, 500, 2, batch_short=True) == []


def test_batch_short_needs_a_model_forward_varlen_knows():
    """... at construction, and before the device check."""
    import torch
    from taiyaki_amd import basecall, layers, models

    class Other(torch.nn.Module):
        def forward(self, x):
            return x

    for bad in (Other(), layers.Serial([layers.Convolution(1, 8, 5, stride=5), torch.nn.Tanh()])):
        with pytest.raises(TypeError):
            basecall.Basecaller(bad, stride=5, batch_short=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):     # a model it knows, on the CPU: the usual refusal
        basecall.Basecaller(models.mLstm_flipflop(size=16, stride=5), batch_short=True)


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _models(dev):
    """The seeded networks of tests/test_basecall_reads.py."""
    import torch
    from taiyaki_amd import models, synth
    torch.manual_seed(13)
    gru = models.mGru_flipflop(size=96, stride=2).to(dev).eval()
    torch.manual_seed(14)
    lstm = models.mLstm_flipflop(size=64, stride=5).to(dev).eval()
    return {"gru": (synth.excite_network(gru), 2), "lstm": (synth.excite_network(lstm), 5)}


def _reads(stride):
    """Reads 1, 3, 5, 6 and 7 are shorter than a chunk at stride 5; at stride 2 (a chunk of 2000 samples) 3, 5 and 6."""
    del stride
    rs = np.random.RandomState(61)
    seeded = [(90 + 12 * rs.standard_normal(n) + 3 * np.sin(np.arange(n) / 300.0)).astype(np.float32) for n in (1234, 4321)]
    return [bs.signal("len9500"), bs.signal("len4999"), np.zeros(0, dtype=np.float32), bs.signal("len2"),
            bs.signal("len23456"), bs.signal("len1"), seeded[0], seeded[1]]


def _qstring(err, qs, qo):
    """The header's quality characters (include/taiyaki_amd_basecall.h (c)): numpy's float32 arithmetic, one operation
    at a time, '!' for a NaN or a code below it, '~' above."""
    with np.errstate(all="ignore"):
        code = ((np.float32(qs) * (np.float32(-10.0) * np.log10(err.astype(np.float32))) + np.float32(qo)) + np.float32(33)) + np.float32(0.5)
    low, high = ~(code >= 33), code >= 127
    out = np.where(low | high, 40, code).astype(np.uint8)
    out[low], out[high] = 33, 126
    return out.tobytes().decode("ascii")


def _padded_columns(sigs, reads):
    """What tk_basecall_gather_columns_dev gives for these reads with the device's median / MAD (bit for bit: the gather
    and med / MAD tests) -> (x (tmax, ncol, 1), lengths, refused)."""
    from taiyaki_amd import clipping
    lens = [len(sigs[r]) for r in reads]
    x, refused = np.zeros((max(lens), len(reads), 1), dtype=np.float32), []
    for j, r in enumerate(reads):
        med, mad = clipping.med_mad(sigs[r])
        refused.append(not mad > 0)
        if mad > 0:
            x[:lens[j], j, 0] = ((sigs[r] - med) / mad).astype(np.float32)
    return x, lens, refused


def _expected_short(model, stride, chunk_blocks, sigs, width, dev, posterior=True, temperature=1.0, fastq=False,
                    qs=1.0, qo=0.0, beam=None):
    """{read: (sequence, quality string or None, nsamples, path, categorical rows)} of the reads shorter than a chunk,
    grouped as the plan groups them."""
    import torch
    from taiyaki_amd import decode, decodeutil, flipflopfings, layers, qscores
    short = [r for r, x in enumerate(sigs) if 0 < len(x) < chunk_blocks * stride]
    want = {}
    for k in range(0, len(short), width):
        reads = short[k:k + width]
        x, lens, refused = _padded_columns(sigs, reads)
        with torch.no_grad():
            out, out_lens = layers.forward_varlen(model, torch.from_numpy(x).to(dev), lens)
            scores = (out[:, :, :40] * temperature).contiguous()
            if posterior:
                batch_post = decode.flipflop_make_trans(scores, lengths=[int(n) for n in out_lens])
            for j, r in enumerate(reads):
                if refused[j]:
                    want[r] = ("", "" if fastq else None, lens[j], None, None)
                    continue
                L = int(out_lens[j])
                trans = scores[:L, j:j + 1].contiguous()
                if posterior:
                    trans = (batch_post[:L, j:j + 1].contiguous() + 1e-8).log()
                if beam:
                    best, _ = decodeutil.beamsearch(trans[:, 0].contiguous(), 0.0, beam[0], beam[1])
                    want[r] = (flipflopfings.path_to_str(best, alphabet="ACGT", include_first_source=False), None, lens[j], None, None)
                    continue
                path = decode.flipflop_viterbi_path(trans)                  # the existing fixed-length operator
                seq, _, sp = bs.tail(path.cpu().numpy(), None, [0], [lens[j]], stride)
                q = None
                if fastq:
                    err = qscores.errprobs_from_trans(trans, path).cpu().numpy()[:, 0]
                    q = _qstring(err[1:][sp[1:] != sp[:-1]], qs, qo)
                want[r] = (seq, q, lens[j], sp, out[:L, j, 40:].cpu().numpy())
    return want


@pytest.mark.gpu
@pytest.mark.parametrize("width", [2, 16])
@pytest.mark.parametrize("which", ["gru", "lstm"])
def test_batched_short_reads_equal_the_chain_on_their_columns(gpu_device, which, width):
    from taiyaki_amd import basecall
    model, stride = _models(gpu_device)[which]
    sigs = _reads(stride)
    chunk = bs.CHUNK_BLOCKS * stride
    short = [r for r, x in enumerate(sigs) if 0 < len(x) < chunk]
    assert len(short) > width or width == 16
    for posterior, fastq in itertools.product((True, False), (True, False)):
        kw = dict(chunk_size=bs.CHUNK_BLOCKS, overlap=bs.OVERLAP_BLOCKS, max_concurrent_chunks=width, posterior=posterior,
                  temperature=0.7, fastq=fastq, qscore_scale=0.9, qscore_offset=0.3)
        got = basecall.Basecaller(model, batch_short=True, **kw).call(sigs)
        alone = basecall.Basecaller(model, batch_short=False, **kw).call(sigs)
        want = _expected_short(model, stride, bs.CHUNK_BLOCKS, sigs, width, gpu_device, posterior, 0.7, fastq, 0.9, 0.3)
        assert sorted(want) == short and [g[2] for g in got] == [len(x) for x in sigs]
        tag = (which, width, posterior, fastq)
        for r in range(len(sigs)):
            if r in want:
                seq, q, nsample = got[r]
                assert seq == want[r][0] and nsample == want[r][2], (tag, r)
                if fastq:
                    assert len(q) == len(seq) and bs.qstrings_close(q, want[r][1]), (tag, r)
                else:
                    assert q is None
            else:
                assert got[r] == alone[r], (tag, r)                 # the reads of a chunk or more, and the empty one
        assert got[2] == ("", "" if fastq else None, 0) and got[5][0] == ""       # no samples; MAD == 0
        # the two longest short reads call bases (at stride 2 the second longest has two samples: one block)
        by_length = [r for r in sorted(short, key=lambda r: -len(sigs[r]))[:2] if len(sigs[r]) > 100]
        assert by_length and all(len(got[r][0]) > 0 for r in by_length), tag
        # against every short read called alone: the network's GEMMs have another shape, so only well-formedness holds
        same = sum(got[r][0] == alone[r][0] for r in short)
        for r in short:
            a, b = got[r][0], alone[r][0]
            differing = sum(x != y for x, y in zip(a, b)) + abs(len(a) - len(b))
            assert got[r][2] == alone[r][2] and abs(len(a) - len(b)) <= differing
        print("%s width %d posterior %s fastq %s: %d of %d short reads have the sequence they get alone; bases %s"
              % (which, width, posterior, fastq, same, len(short), [len(got[r][0]) for r in short]))


def _count_calls(monkeypatch, model):
    from taiyaki_amd import basecall
    columns, passes = [], []
    forward, varlen = model.forward, basecall.layers.forward_varlen
    monkeypatch.setattr(model, "forward", lambda x: (columns.append(x.shape[1]), forward(x))[1])
    monkeypatch.setattr(basecall.layers, "forward_varlen", lambda m, x, n: (passes.append(x.shape[1]), varlen(m, x, n))[1])
    return columns, passes


@pytest.mark.gpu
def test_one_network_pass_per_short_slice(gpu_device, monkeypatch):
    from taiyaki_amd import basecall
    model, stride = _models(gpu_device)["lstm"]
    sigs = _reads(stride)
    batch = [sigs[1], sigs[3], sigs[6], sigs[7]]                    # four short reads
    # (the stride is given: guessing it at construction is a pass of the model on one column, which is not a call's)
    kw = dict(stride=stride, chunk_size=bs.CHUNK_BLOCKS, overlap=bs.OVERLAP_BLOCKS)
    columns, passes = _count_calls(monkeypatch, model)
    basecall.Basecaller(model, batch_short=True, max_concurrent_chunks=16, **kw).call(batch)
    assert columns.count(1) == 0 and passes == [4]
    del columns[:], passes[:]
    basecall.Basecaller(model, batch_short=True, max_concurrent_chunks=3, **kw).call(batch)
    assert columns.count(1) == 0 and passes == [3, 1]
    del columns[:], passes[:]
    basecall.Basecaller(model, batch_short=False, max_concurrent_chunks=16, **kw).call(batch)
    assert columns.count(1) == 4 and passes == []


@pytest.mark.gpu
def test_call_mods_of_batched_short_reads(gpu_device):
    """The short reads' score rows are numpy's extract_mod_weights (tests/mods_support.py) on the column's own path and
    categorical rows, bit for bit; the calls are `call`'s."""
    import torch
    from taiyaki_amd import basecall, models, synth
    torch.manual_seed(21)
    net = synth.excite_network(models.mLstm_cat_mod_flipflop(size=32, stride=5, can_nmods=(1, 1, 0, 0))).to(gpu_device).eval()
    rs = np.random.RandomState(41)
    sigs = [(90 + 12 * rs.standard_normal(n)).astype(np.float32) for n in (2077, 503, 2, 0, 777, 999, 1850)]
    kw = dict(chunk_size=200, overlap=20, max_concurrent_chunks=3, fastq=True)
    caller = basecall.Basecaller(net, mod_output=True, batch_short=True, **kw)
    results, mods = caller.call_mods(sigs)
    assert results == caller.call(sigs) and [r[2] for r in results] == [len(x) for x in sigs]
    plain = basecall.Basecaller(net, mod_output=True, **kw).call_mods(sigs)
    want = _expected_short(net, 5, 200, sigs, 3, gpu_device, fastq=True)
    assert sorted(want) == [1, 2, 4, 5]
    for r, (seq, q, _) in enumerate(results):
        m = mods[r]
        assert m.dtype == np.float32 and m.shape == (len(seq), 2) and len(q) == len(seq)
        if r in want:
            assert seq == want[r][0] and bs.qstrings_close(q, want[r][1])
            assert ms.same_bits(m, ms.moves_to_mods(want[r][4], want[r][3], (1, 1, 0, 0))), r
        else:
            assert (seq, q) == plain[0][r][:2] and ms.same_bits(m, plain[1][r]), r
        letters = np.frombuffer(seq.encode(), dtype=np.uint8)
        assert np.array_equal(~np.isnan(m), np.stack([letters == ord("A"), letters == ord("C")], axis=1))
    assert min(len(results[r][0]) for r in (1, 4, 5)) > 20          # (not a comparison of empty calls)


@pytest.mark.gpu
@pytest.mark.parametrize("posterior", [True, False])
def test_beam_on_batched_short_reads(gpu_device, posterior):
    """Every short read's call is decodeutil.beamsearch on that read's own rows of the same scores."""
    from taiyaki_amd import basecall
    model, stride = _models(gpu_device)["lstm"]
    sigs = _reads(stride)
    kw = dict(chunk_size=bs.CHUNK_BLOCKS, overlap=bs.OVERLAP_BLOCKS, max_concurrent_chunks=2, posterior=posterior,
              temperature=0.7, beam=(5, True))
    got = basecall.Basecaller(model, batch_short=True, **kw).call(sigs)
    alone = basecall.Basecaller(model, **kw).call(sigs)
    want = _expected_short(model, stride, bs.CHUNK_BLOCKS, sigs, 2, gpu_device, posterior, 0.7, beam=(5, True))
    assert sorted(want) == [1, 3, 5, 6, 7]
    for r in range(len(sigs)):
        assert got[r] == (want[r][:3] if r in want else alone[r]), r
    assert len(got[1][0]) > 0 and len(got[7][0]) > 0 and got[2] == ("", None, 0)
