"""Chunks of a fixed number of bases on the GPU (csrc/chunk_seqlen.hip through include/taiyaki_amd_chunks_seqlen.h,
`MappedSignalStore.sample_sequence_chunks`, `train.SquiggleTrainer`): against the fixture the genuine reference wrote
(tests/golden/chunks_seqlen.npz) and, beyond it, against the numpy restatement that tests/test_chunks_seqlen_host.py pins
to that fixture -- bit for bit: the signal is float64 arithmetic rounded once to float32, everything else is integer work
or a table look-up."""
import copy
import os

import numpy as np
import pytest

from tests import chunks_seqlen_support as support
from tests.chunks_seqlen_support import REASONS, ReplayRng, fields, same, same_bits
from tests.golden.make_golden_chunks_seqlen import FORMS, SPECS, spec_reads

pytestmark = pytest.mark.gpu
CASES = [(name, form) for name in sorted(SPECS) for form in FORMS]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "chunks_seqlen.npz"))


def host(t):
    return t.cpu().numpy()


def check_batch(b, chunks, counts, attempts, nwant, bases, reverse):
    """Every field of a SquiggleChunkBatch against the restatement's accepted chunks."""
    n = b.naccepted
    assert n == len(chunks) and b.attempts == attempts
    assert b.rejections() == {k: v for k, v in counts.items() if v}
    sel = b.sel[:n].long()
    assert same(host(b.sel[n:]), np.full(nwant - n, -1))
    assert same(host(b.cand_read[sel]), [c["read"] for c in chunks])
    assert same(host(b.dacstart[sel]), [c["start"] for c in chunks])
    assert same(host(b.refstart[sel]), [c["refstart"] for c in chunks])
    assert same(host(b.maxdwell[sel]), [c["max_dwell"] for c in chunks])
    seq_embed, signal, siglens, seqs = support.assemble_batch(chunks, reverse=reverse)
    total = int(siglens.sum())
    assert b.seq_embed.shape == (bases, nwant, 3) and b.seqs.shape == (bases, nwant) and b.siglens.shape == (nwant,)
    assert same(host(b.sigoff), np.concatenate([[0], np.cumsum(siglens), np.full(nwant - n, total)]))
    assert same(host(b.siglens[:n]), siglens) and same_bits(host(b.signal[:total]), signal)
    assert same(host(b.seqs[:, :n]), seqs) and same_bits(host(b.seq_embed[:, :n]), seq_embed)
    # zeros beyond the accepted count and beyond sigoff[n]
    assert b.signal.numel() >= total and not b.signal[total:].any() and not b.siglens[n:].any()
    assert not b.seqs[:, n:].any() and not b.seq_embed[:, n:].any()
    got = b.trimmed()
    assert same_bits(host(got[0]), seq_embed) and same_bits(host(got[1]), signal) and same(host(got[2]), siglens)
    assert got[0].is_contiguous() and got[0].shape[1] == n


# ---------------------------------------------------------------------------------------------
# 1. the fixture: the reference's own chunks
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name, form", CASES)
def test_batches_are_the_reference(golden, gpu_device, name, form):
    from taiyaki_amd import mapped_signal as ms
    spec, g = SPECS[name], fields(golden, name, form)
    reads = spec_reads(spec)
    store = ms.MappedSignalStore(reads, gpu_device)
    fp = store.sample_filter_parameters(spec["nsample"], spec["bases"], spec["filter_mean_dwell"],
                                        spec["filter_max_dwell"], spec["min_pass"], spec["stride"], spec["path_buffer"],
                                        rng=ReplayRng(g["draws_filter"]), chunk_len_means_sequence_len=(form == "seq"))
    assert (fp.median_meandwell, fp.mad_meandwell) == tuple(g["median_mad"])
    n = len(g["chunk_read"])
    for tag, rev in (("fwd", False), ("rev", True)):
        if rev:     # ... and through the flip-flop producer's front door
            b = store.sample_chunks(spec["nwant"], spec["bases"], fp, reverse=True, rng=ReplayRng(g["draws_batch"]),
                                    chunk_len_means_sequence_len=True)
        else:
            b = store.sample_sequence_chunks(spec["nwant"], spec["bases"], fp, rng=ReplayRng(g["draws_batch"]))
        assert isinstance(b, ms.SquiggleChunkBatch)
        rej = b.rejections()
        assert [rej.get(k, 0) for k in REASONS] == list(g["rejections"])
        assert b.naccepted == n and b.attempts == int(g["rejections"].sum())
        sel = b.sel[:n].long()
        assert same(host(b.cand_read[sel]), g["chunk_read"]) and same(host(b.dacstart[sel]), g["chunk_start"])
        assert same(host(b.maxdwell[sel]), g["chunk_maxdwell"]) and same(host(b.siglens[:n]), g["chunk_siglen"])
        total = int(g["chunk_siglen"].sum())
        assert int(b.sigoff[n]) == total == int(b.sigoff[-1])
        assert same_bits(host(b.signal[:total]), g["signal_" + tag])
        assert same(host(b.seqs[:, :n]), g["seqs_" + tag]) and same_bits(host(b.seq_embed[:, :n]), g["embed_" + tag])
        assert not b.signal[total:].any() and not b.siglens[n:].any()
        assert not b.seqs[:, n:].any() and not b.seq_embed[:, n:].any()
        seq_embed, signal, siglens = b.trimmed()        # the reference's batch (bin/train_squiggle.py:201-209)
        assert same_bits(host(seq_embed), g["embed_" + tag]) and same_bits(host(signal), g["signal_" + tag])
        assert same(host(siglens), g["chunk_siglen"])
        assert signal.numel() == total and seq_embed.shape[:2] == (spec["bases"], n)


# ---------------------------------------------------------------------------------------------
# 2. the trainer's own shape, candidates drawn on the device
# ---------------------------------------------------------------------------------------------
TRAINER_BASES, TRAINER_CHUNKS = 300, 100


@pytest.fixture(scope="module")
def trainer_reads():
    from taiyaki_amd import synth
    return synth.mapped_reads(200, 181, mean_reflen=1500, long_dwell_prob=0.002)


@pytest.fixture(scope="module")
def trainer_store(trainer_reads, gpu_device):
    import torch
    from taiyaki_amd import mapped_signal as ms
    store = ms.MappedSignalStore(trainer_reads, gpu_device)
    torch.manual_seed(11)
    fp = store.sample_filter_parameters(1000, TRAINER_BASES, 3.0, 10.0, 0.5, 1, 1.1, chunk_len_means_sequence_len=True)
    return store, fp


def restated(reads, b, nwant, bases, fp, standardize=True):
    """The restatement on the candidates a batch was drawn with, whichever way they were drawn: read back as
    (read, refstart - region start); a read without spare length is tooshort at any start."""
    cr, refstart = host(b.cand_read), host(b.refstart)
    cands = []
    for k, rn in enumerate(cr):
        lo, hi = support.mapped_reference_region(reads[rn])
        cands.append((int(rn), int(refstart[k]) - lo if hi - lo - bases > 0 else 0))
    return support.sample_chunks(reads, nwant, bases, dict(fp._asdict()), cands, standardize)


def test_trainer_shape_with_device_drawn_candidates(trainer_reads, trainer_store):
    import torch
    store, fp = trainer_store
    assert 5.0 < fp.median_meandwell < 15.0 and fp.mad_meandwell > 0
    torch.manual_seed(12)
    b = store.sample_sequence_chunks(TRAINER_CHUNKS, TRAINER_BASES, fp)
    chunks, counts, attempts = restated(trainer_reads, b, TRAINER_CHUNKS, TRAINER_BASES, fp)
    assert len(chunks) > TRAINER_CHUNKS // 2 and len(counts) > 2         # (a real batch, with rejections)
    check_batch(b, chunks, counts, attempts, TRAINER_CHUNKS, TRAINER_BASES, False)
    # the draw covers the spare length: starts near both of its ends occur
    lo = store.mapped_ref[host(b.cand_read), 0]
    spare = store.mapped_ref[host(b.cand_read), 1] - lo - TRAINER_BASES
    frac = (host(b.refstart) - lo)[spare > 0] / spare[spare > 0]
    assert frac.min() >= 0 and frac.max() < 1 and frac.min() < 0.1 and frac.max() > 0.9
    # read by read, and reversed
    b = store.sample_sequence_chunks(TRAINER_CHUNKS, TRAINER_BASES, fp, select_strands_randomly=False,
                                     first_strand_index=197, reverse=True)
    assert list(host(b.cand_read[:5])) == [197, 198, 199, 0, 1]
    chunks, counts, attempts = restated(trainer_reads, b, TRAINER_CHUNKS, TRAINER_BASES, fp)
    check_batch(b, chunks, counts, attempts, TRAINER_CHUNKS, TRAINER_BASES, True)


# ---------------------------------------------------------------------------------------------
# 3. standardize=False, explicit candidates
# ---------------------------------------------------------------------------------------------
def test_raw_current_and_explicit_candidates(gpu_device):
    from taiyaki_amd import mapped_signal as ms
    spec = SPECS["r40b60"]
    reads = spec_reads(spec)
    store = ms.MappedSignalStore(reads, gpu_device)
    bases, nwant = 37, 70            # (more than one workgroup of candidates, a column count that is no multiple of 64)
    rng = np.random.RandomState(5)
    cr = rng.randint(0, len(reads), 100)
    spare = store.mapped_ref[cr, 1] - store.mapped_ref[cr, 0] - bases
    cs = (rng.uniform(0, 1, 100) * np.maximum(spare, 1)).astype(np.int64)
    cs[::9] = spare[::9]            # start == spare: too short
    cs[4::11] = spare[4::11] - 1    # the last start there is (or -1 on a read without spare length)
    for fp in (ms.FILTER_PARAMETERS(3.0, 10.0, 0.7, None, None, None, None),
               ms.FILTER_PARAMETERS(2.0, 5.0, 0.7, 8.5, 1.3, 1, 1.1)):
        for rev in (False, True):
            b = store.sample_sequence_chunks(nwant, bases, fp, standardize=False, reverse=rev, candidates=(cr, cs))
            want = support.sample_chunks(reads, nwant, bases, dict(fp._asdict()), list(zip(cr, np.maximum(cs, 0))),
                                         standardize=False)
            assert want[1].get("tooshort", 0) >= 11 and len(want[0]) >= 30
            check_batch(b, *want, nwant, bases, rev)
    # raw current: no shift, no scale
    r = reads[want[0][0]["read"]]
    a = want[0][0]["start"]
    raw = ((r["Dacs"][a:a + 5] + r["offset"]) * r["range"] / r["digitisation"]).astype(np.float32)
    assert same_bits(host(b.signal[:b.siglens[0]].flip(0)[:5]), raw)


# ---------------------------------------------------------------------------------------------
# 4. starvation, emptiness, a buffer too small
# ---------------------------------------------------------------------------------------------
def test_starvation_unmapped_reads_and_small_buffers(gpu_device):
    import torch
    from taiyaki_amd import mapped_signal as ms, synth
    reads = synth.mapped_reads(5, 93, mean_reflen=30)
    nofilter = ms.FILTER_PARAMETERS(3.0, 10.0, 0.25, None, None, None, None)
    store = ms.MappedSignalStore(reads, gpu_device)
    b = store.sample_sequence_chunks(8, 100000, nofilter)
    assert b.naccepted == 0 and b.rejections() == {"tooshort": 32} and b.attempts == 32
    assert not b.signal.any() and not b.siglens.any() and not b.seqs.any() and not b.seq_embed.any()
    assert not b.sigoff.any() and b.seqs.shape == (100000, 8)
    seq_embed, signal, siglens = b.trimmed()
    assert seq_embed.shape == (100000, 0, 3) and signal.numel() == 0 and siglens.numel() == 0
    # filters off: the buffer holds the longest mapped span of any read, per chunk
    assert b.signal.numel() == 8 * int((store.mapped[:, 1] - store.mapped[:, 0]).max())
    # a read with nothing mapped beside one that is; a slip (two bases on one sample) as a chunk of its own
    dacs = (np.arange(300) % 97).astype(np.int16)
    scale = dict(offset=1.0, range=2.0, digitisation=4.0, shift_frompA=0.5, scale_frompA=3.0)
    none = dict(read_id="none", Dacs=dacs, Reference=np.array([1, 2], dtype=np.int16),
                Ref_to_signal=np.array([-1, 301, 301], dtype=np.int32), **scale)
    one = dict(read_id="one", Dacs=dacs, Reference=np.array([2, 2, 3, 0, 1], dtype=np.int16),
               Ref_to_signal=np.array([-1, 10, 10, 250, 260, 301], dtype=np.int32), **scale)
    s2 = ms.MappedSignalStore([none, one], gpu_device)
    assert [list(x) for x in s2.mapped_ref] == [[0, 0], [1, 4]]
    cands = ([0, 1, 1, 1, 1], [0, 0, 1, 2, 5])
    b = s2.sample_sequence_chunks(5, 1, nofilter, candidates=cands)
    # (read `none`: too short; base 1: no samples; base 2: 240 samples; base 3 would need the region's last index)
    assert b.rejections() == {"pass": 1, "emptysignal": 1, "tooshort": 3} and b.naccepted == 1
    want = support.sample_chunks([none, one], 5, 1, dict(nofilter._asdict()), list(zip(*cands)))
    check_batch(b, *want, 5, 1, False)
    assert list(host(b.siglens)) == [240, 0, 0, 0, 0] and int(b.seqs[0, 0]) == 3 and int(b.maxdwell[b.sel[0]]) == 1
    assert same_bits(host(b.signal[:240]), ((((dacs[10:250] + 1.0) * 2.0 / 4.0) - 0.5) / 3.0).astype(np.float32))
    b = s2.sample_sequence_chunks(2, 2, nofilter, candidates=([1, 1], [0, 0]))
    assert b.naccepted == 2 and list(host(b.siglens)) == [240, 240] and list(host(b.maxdwell)) == [0, 0]
    # a buffer too small for the batch: the status word says so, and the chunks that fit are whole
    spec = SPECS["r40b60"]
    reads = spec_reads(spec)
    store = ms.MappedSignalStore(reads, gpu_device)
    cr, cs = np.arange(len(reads)), np.zeros(len(reads), dtype=np.int64)
    full = store.sample_sequence_chunks(12, 60, nofilter, candidates=(cr, cs))
    lens = host(full.siglens)
    assert full.naccepted == 12 and lens.min() > 0
    per_chunk = int(np.cumsum(lens)[7] // 12) + 1       # 12 * per_chunk samples: eight chunks fit, the ninth does not
    assert np.cumsum(lens)[7] <= 12 * per_chunk < np.cumsum(lens)[8]
    small = store.sample_sequence_chunks(12, 60, nofilter, candidates=(cr, cs), max_samples_per_chunk=per_chunk)
    with pytest.raises(RuntimeError, match="max_samples_per_chunk"):
        small.naccepted
    with pytest.raises(RuntimeError, match="max_samples_per_chunk"):
        small.trimmed()
    fit = int(np.cumsum(lens)[7])
    assert small.signal.numel() == 12 * per_chunk
    assert same_bits(host(small.signal[:fit]), host(full.signal[:fit])) and not small.signal[fit:].any()
    assert same(host(small.siglens), lens) and same(host(small.seqs), host(full.seqs))
    # the store checks its reads as before
    with pytest.raises(ValueError, match="one longer"):
        ms.MappedSignalStore([dict(one, Ref_to_signal=np.array([0, 5, 9], dtype=np.int32))], gpu_device)
    with pytest.raises(ValueError, match="monotonically"):
        ms.MappedSignalStore([dict(one, Ref_to_signal=np.array([0, 5, 3, 9, 9, 9], dtype=np.int32))], gpu_device)
    # a training set with more than four labels is refused: the embedding has four rows
    with pytest.raises(ValueError, match="four bases"):
        ms.MappedSignalStore(synth.mapped_reads(3, 5, nlabel=6), gpu_device).sample_sequence_chunks(2, 5, nofilter)
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------
# 5. the reference's real reads
# ---------------------------------------------------------------------------------------------
def test_real_reads_from_hdf5(gpu_device):
    from taiyaki_amd import hdf5_lite, mapped_signal as ms
    path = os.path.join(GOLDEN, "mapped_signal", "mapped_reads_0.hdf5")
    _, reads = hdf5_lite.read_mapped_signal_file(path)
    store = ms.MappedSignalStore.from_hdf5(path, gpu_device)
    rs = np.random.RandomState(3)
    fp = store.sample_filter_parameters(50, 30, 3.0, 10.0, 0.5, 1, 1.1, rng=rs, chunk_len_means_sequence_len=True)
    assert fp.median_meandwell > 1.1 and fp.mad_meandwell > 0
    for rev in (False, True):
        b = store.sample_sequence_chunks(40, 30, fp, rng=rs, reverse=rev)
        chunks, counts, attempts = restated(reads, b, 40, 30, fp)
        assert len(chunks) >= 20
        check_batch(b, chunks, counts, attempts, 40, 30, rev)


# ---------------------------------------------------------------------------------------------
# 6. the batch feeds the loss
# ---------------------------------------------------------------------------------------------
def loss_and_grads(net, seq_embed, signal, siglens):
    import torch
    from taiyaki_amd.squiggle_match import squiggle_match_loss
    net.zero_grad()
    loss = squiggle_match_loss(net(seq_embed), signal, siglens, 1e-15)
    (loss.sum() / siglens.sum()).backward()
    assert torch.isfinite(loss).all() and all(torch.isfinite(p.grad).all() for p in net.parameters())
    return [host(loss.detach())] + [host(p.grad) for p in net.parameters()]


def test_batch_feeds_the_loss(trainer_reads, trainer_store, gpu_device):
    import torch
    from taiyaki_amd import layers, models
    store, fp = trainer_store
    torch.manual_seed(13)
    net = models.squiggle_predictor(32, 4, 9).to(gpu_device)
    b = store.sample_sequence_chunks(24, TRAINER_BASES, fp)
    calls = dict(layers.SQUIGGLE_NET_LAUNCHES)
    got = loss_and_grads(net, *b.trimmed())
    assert layers.SQUIGGLE_NET_LAUNCHES == {k: v + 1 for k, v in calls.items()}      # (the network's own kernels)
    # the same chunks assembled on the host, the reference's way, and uploaded
    chunks, _, _ = restated(trainer_reads, b, 24, TRAINER_BASES, fp)
    assert len(chunks) == b.naccepted > 8
    seq_embed, signal, siglens, _ = support.assemble_batch(chunks)
    want = loss_and_grads(net, *(torch.from_numpy(x).to(gpu_device) for x in (seq_embed, signal, siglens)))
    assert len(got) == len(want) == 1 + 2 * 6
    for g, w in zip(got, want):
        assert same_bits(g, w)


# ---------------------------------------------------------------------------------------------
# 7. the trainer's step
# ---------------------------------------------------------------------------------------------
def test_squiggle_trainer_step(trainer_store, gpu_device):
    import torch
    from taiyaki_amd import models, train
    from taiyaki_amd.squiggle_match import squiggle_match_loss
    store, fp = trainer_store
    torch.manual_seed(14)
    net = models.squiggle_predictor(32, 4, 9).to(gpu_device)
    twin = copy.deepcopy(net)
    trainer = train.SquiggleTrainer(net)
    b = store.sample_sequence_chunks(16, TRAINER_BASES, fp)
    fval = trainer.step(b)
    assert fval.is_cuda and fval.ndim == 0 and bool(torch.isfinite(fval))
    # the step written out by hand (bin/train_squiggle.py:165-171, 216-224) on the twin
    opt = torch.optim.AdamW(twin.parameters(), lr=1e-4, betas=(0.9, 0.999), weight_decay=0.0, eps=1e-6, capturable=True)
    seq_embed, signal, siglens = b.trimmed()
    opt.zero_grad()
    want = squiggle_match_loss(twin(seq_embed), signal, siglens, 1e-15).sum() / siglens.sum()
    want.backward()
    opt.step()
    assert same_bits(host(fval).reshape(1), host(want.detach()).reshape(1))
    assert len(list(net.parameters())) == 12
    for p, q in zip(net.parameters(), twin.parameters()):
        assert same_bits(host(p.detach()), host(q.detach()))
    before = [host(p.detach()).copy() for p in net.parameters()]
    # a triple steps like a batch; the learning rate follows lr_max * lr_decay / (i + lr_decay)
    trainer.step(b.trimmed())
    trainer.step((seq_embed, signal, siglens))
    assert any(not np.array_equal(x, host(p.detach())) for x, p in zip(before, net.parameters()))
    assert trainer.opt.param_groups[0]["lr"] == 1e-4 * (5000 / (3 + 5000))
    assert train.SquiggleTrainer(twin, lr_max=2e-3, lr_decay=10).opt.param_groups[0]["lr"] == 2e-3
