"""Basecall batches of reads on the device: raw float32 signals in, sequences and quality strings out
(``bin/basecall.py:151-242``: the Viterbi path, `posterior` on or off, or -- ``beam=(width, guided)`` -- the hash beam
search on every read's stitched transition scores).

Between the upload of the signals and the download of the finished characters nothing runs on the host: median / MAD
normalisation, chunking and the tail (stitch, collapse, quality characters) are the three kernels of
include/taiyaki_amd_basecall.h; the network, `flipflop_make_trans`, the Viterbi and `errprobs_from_trans` are the
operators this package already has.  `call_mods` adds, for a cat-mod model, the modified-base scores of every called
base (tk_basecall_mod_weights_dev on the Viterbi paths and the network's categorical columns), in the same download.
With a beam, the stitched scores of all the batch's reads (tk_basecall_stitch_scores_dev) go through ONE launch of the
beam search (tk_basecall_beamsearch_dev), which writes the calls.  There is no CPU fallback: a model that is not on an
AMD GPU raises.
"""
import collections
import ctypes
import types

import numpy as np
import torch

from taiyaki_amd import _lib, basecall_helpers, decode, decodeutil, flipflopfings, layers, qscores

Beam = collections.namedtuple("Beam", "width guided")       # bin/basecall.py's --beam
Slice = collections.namedtuple("Slice", "short first ncol reads")
Slice.__doc__ = """One model invocation of the packing plan: `ncol` columns.  short=False: columns [first, first + ncol)
of the batch's chunk tensor; short=True: reads shorter than a chunk, each one chunk of its own length -- read `first`
alone, or (batch_short) the reads `reads` as zero-padded columns of one tensor.  `reads`: the read of every column."""


def chunk_counts(lengths, chunk_size, overlap):
    """Chunks per read in the batch's chunk tensor (samples): the closed form of basecall_helpers.chunk_read's count,
    0 for a read shorter than `chunk_size` (it is called alone, as one chunk of its own length)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    step = chunk_size - overlap
    return np.where(lengths < chunk_size, 0, (lengths - chunk_size + step - 1) // step + 1)


def packing_plan(lengths, chunk_size, overlap, max_concurrent_chunks, pack=True, batch_short=False):
    """The model invocations for reads of `lengths` samples, host arithmetic on lengths alone.  Every chunk appears
    once, in read order; no slice is wider than `max_concurrent_chunks`.  pack=True fills every slice across read
    boundaries; pack=False splits per read, as `torch.split` does in bin/basecall.py:208.  Reads shorter than
    `chunk_size` follow as slices of one column each (reads without samples get none) or -- batch_short -- in read
    order as slices of up to `max_concurrent_chunks` columns."""
    counts = chunk_counts(lengths, chunk_size, overlap)
    owner = np.repeat(np.arange(len(counts)), counts)
    plan = []
    if pack:
        bounds = [(0, len(owner))]
    else:
        off = np.concatenate([[0], np.cumsum(counts)])
        bounds = [(int(off[r]), int(off[r + 1])) for r in range(len(counts)) if counts[r]]
    for lo, hi in bounds:
        for first in range(lo, hi, max_concurrent_chunks):
            ncol = min(max_concurrent_chunks, hi - first)
            plan.append(Slice(False, first, ncol, tuple(int(r) for r in owner[first:first + ncol])))
    short = [r for r, n in enumerate(lengths) if 0 < n < chunk_size]
    width = max_concurrent_chunks if batch_short else 1
    for k in range(0, len(short), width):
        plan.append(Slice(True, short[k], len(short[k:k + width]), tuple(short[k:k + width])))
    return plan


def stitched_rows(nchunks, siglen, chunk_size, overlap, stride, nrow):
    """Rows that basecall_helpers.stitch_chunks keeps of a read's `nchunks` chunks of `nrow` rows each: the bound of
    the read's call length."""
    if nchunks <= 1:
        return nrow * nchunks
    starts, ends = basecall_helpers.chunk_bounds(siglen, chunk_size, overlap)
    lo = np.concatenate([[starts[0] // stride], (ends[:-1] - starts[1:]) // (2 * stride)])
    hi = np.concatenate([[(ends[0] + starts[1]) // (2 * stride)],
                         (ends[1:-1] + starts[2:] - 2 * starts[1:-1]) // (2 * stride),
                         [(ends[-1] - starts[-1]) // stride]])
    return int(np.maximum(np.minimum(hi, nrow) - np.minimum(lo, nrow), 0).sum())


def check_beam(beam, beam_cut, nbase, fastq):
    """`Basecaller`'s beam arguments -> Beam(width, guided), or None.  ValueError for a beam together with fastq (the
    reference has no quality string for a beam call), for a width outside the search's admission rule (1..12 with
    width * (nbase + 1) <= 64; nbase 1..4) and for a beam_cut outside [0, 1]."""
    if beam is None:
        return None
    if fastq:
        raise ValueError("Basecaller: beam search gives no quality string (fastq=True needs beam=None)")
    try:
        width, guided = beam
    except (TypeError, ValueError):
        raise ValueError("Basecaller: beam is (width, guided), got %r" % (beam,)) from None
    decodeutil.check_beam(nbase, width, beam_cut, "Basecaller")
    return Beam(int(width), bool(guided))


def check_mods(model, mod_output, beam, nbase):
    """`Basecaller`'s mod_output argument -> the model's can_nmods as a list, or None.  ValueError for mod_output
    together with a beam (the search's states are not per chunk), on a model whose last layer is not
    GlobalNormFlipFlopCatMod, and on one without a modification (or with more than the kernel's
    TK_BASECALL_MAX_NMOD, or whose canonical alphabet is not `nbase` long)."""
    if not mod_output:
        return None
    if beam is not None:
        raise ValueError("Basecaller: mod_output needs the Viterbi path (beam=None); the beam search's states are not "
                         "per chunk")
    if not (isinstance(model, layers.Serial) and layers.is_cat_mod_model(model)):
        raise ValueError("Basecaller: mod_output needs a model whose last layer is GlobalNormFlipFlopCatMod")
    can_nmods = [int(n) for n in model[-1].can_nmods]
    cap = _lib.BASECALL_DEFINES["TK_BASECALL_MAX_NMOD"]
    if sum(can_nmods) == 0:
        raise ValueError("Basecaller: mod_output on a model without a modification (can_nmods %r)" % (can_nmods,))
    if len(can_nmods) != nbase or sum(can_nmods) > cap:
        raise ValueError("Basecaller: can_nmods %r does not fit an alphabet of %d bases and at most %d modifications"
                         % (can_nmods, nbase, cap))
    return can_nmods


def _align(n, to=16):
    return (n + to - 1) // to * to


class _Layout:
    """The byte layout of one transfer: `fields` is an ordered list of (name, dtype, count).  Every field starts on a
    16-byte boundary; `nbytes` ends with the last field.  `view(buf, name)` is that field, typed, of a uint8 numpy
    array or torch tensor that starts with the block (`count`: another number of elements than the field's)."""

    def __init__(self, fields):
        self.fields, self.nbytes = {}, 0
        for name, dtype, count in fields:
            self.fields[name] = (_align(self.nbytes), np.dtype(dtype), count)
            self.nbytes = _align(self.nbytes) + np.dtype(dtype).itemsize * count

    def view(self, buf, name, count=None):
        off, dtype, n = self.fields[name]
        piece = buf[off:off + dtype.itemsize * (n if count is None else count)]
        return piece.view(dtype if isinstance(buf, np.ndarray) else getattr(torch, dtype.name))


def room_offsets(counts, lens, nrow, short, chunk_size, overlap, stride):
    """Where every read's output starts, int64 (nread + 1).  A read's room is its stitched row count, which bounds
    its call length: of `counts[r]` chunks of `nrow` rows each in the batch's chunk tensor, or -- `short`: (read,
    rows) pairs -- the rows of its own chunk; none for a read without samples."""
    rows = np.zeros(len(counts), dtype=np.int64)
    for r in np.flatnonzero(counts):
        rows[r] = stitched_rows(int(counts[r]), int(lens[r]), chunk_size, overlap, stride, nrow)
    for r, n in short:
        rows[r] = n
    return np.concatenate([[0], np.cumsum(rows)]).astype(np.int64)


Segment = collections.namedtuple("Segment", "r0 nread ncol starts ends read_chunk_off nrow path err trans weights "
                                 "rooms rows", defaults=(None, None))
Segment.__doc__ = """A decoded chunk tensor of `ncol` columns and `nrow` rows, and the reads [r0, r0 + nread) it belongs
to: the batch's chunk tensor (r0 = 0, all reads), a short read's own chunk (nread = 1), or -- batch_short -- a slice of
short reads as padded columns (nread = ncol; r0 counts in the call's extended numbering, where the batched short reads
follow the call's reads: see `_upload`).  `path`, `err` (fastq), `weights` (call_mods) on the Viterbi path, `trans` with
a beam; `starts`, `ends`, `read_chunk_off` from the gather.  Padded columns only: `rooms`, every read's room in the
output (host), and `rows`, every column's true row count (device int32)."""


def _at(t, r0):     # &t[r0] of a per-read device array: where a segment's reads start in it
    return _lib._vp(t.data_ptr() + r0 * t.element_size())


class Basecaller:
    """`call(signals)` -> [(sequence, quality string or None, nsamples)] for a batch of reads; with mod_output=True,
    `call_mods(signals)` -> (the same list, [the modified-base scores of every read's call]).

    chunk_size / overlap are in blocks of the model's stride, as on the reference's command line; `stride` is guessed
    from the model when not given (helpers.guess_model_stride).  `reverse`: the signals are reversed before calling
    (the reference's model.metadata['reverse']).  `pack`: fill the model's batches across read boundaries; False
    splits them per read, exactly as the reference's loop does.  `beam`: (width, guided) decodes every read with the
    hash beam search on its stitched scores instead of the Viterbi path (`beam_cut` as decodeutil.beamsearch's); no
    quality strings then.  `mod_output`: the model is a cat-mod model (its last layer GlobalNormFlipFlopCatMod) and
    `call_mods` is wanted; `call` gives what it gives without it.  `batch_short`: the reads shorter than a chunk go
    through the network and the decode operators as zero-padded columns of shared tensors (`layers.forward_varlen`, the
    operators of include/taiyaki_amd_decode_varlen.h), up to max_concurrent_chunks of them at a time, instead of one by
    one; the model must be one `forward_varlen` has a rule for (TypeError otherwise).  The output layer's scores do
    not depend on the batch (include/taiyaki_amd_out_layer.h), nor do those of the layers in front of it in the mGru
    models (tests/test_out_layer.py); a read's call may still differ from the one it gets alone where the network keeps
    a library GEMM that rounds differently at another column count: the strided convolution at sizes outside 192, 256
    and 384."""

    def __init__(self, model, stride=None, chunk_size=1000, overlap=100, max_concurrent_chunks=128, alphabet="ACGT",
                 posterior=True, temperature=1.0, fastq=False, qscore_scale=1.0, qscore_offset=0.0, reverse=False,
                 pack=True, beam=None, beam_cut=0.0, mod_output=False, batch_short=False):
        self.beam, self.beam_cut = check_beam(beam, beam_cut, len(alphabet), fastq), float(beam_cut)
        self.can_nmods = check_mods(model, mod_output, beam, len(alphabet))
        self.batch_short = bool(batch_short)
        if self.batch_short:
            if not isinstance(model, layers.Serial):
                raise TypeError("Basecaller: batch_short needs a layers.Serial that layers.forward_varlen has a rule "
                                "for, not %s" % type(model).__name__)
            # (TypeError for a layer forward_varlen does not know) -> the strides that turn samples into rows
            self._row_strides = [layer.stride for layer, _, _ in layers._varlen_layers(model)
                                 if isinstance(layer, layers.Convolution)]
        self.model = model
        self.device = basecall_helpers.get_model_device(model)
        if self.device.type != "cuda":
            raise RuntimeError("Basecaller: the model is on %s; basecalling only runs as HIP kernels on an AMD GPU "
                               "(no CPU fallback)" % self.device)
        self.stride = int(stride) if stride is not None else basecall_helpers.guess_model_stride(model)
        self.chunk_size, self.overlap = int(chunk_size) * self.stride, int(overlap) * self.stride
        if not 0 <= self.overlap < self.chunk_size:
            raise ValueError("overlap must be smaller than chunk_size")
        self.max_concurrent_chunks = int(max_concurrent_chunks)
        self.alphabet = alphabet.encode("ascii")
        self.n_can_state = flipflopfings.nstate_flipflop(len(alphabet))
        self.posterior, self.temperature, self.fastq = bool(posterior), float(temperature), bool(fastq)
        self.qscore_scale, self.qscore_offset = float(qscore_scale), float(qscore_offset)
        self.reverse, self.pack = bool(reverse), bool(pack)

    def plan(self, lengths):
        return packing_plan(lengths, self.chunk_size, self.overlap, self.max_concurrent_chunks, self.pack,
                            self.batch_short)

    def call(self, signals, read_params=None):
        return self._call(signals, read_params, False)[0]

    def call_mods(self, signals, read_params=None):
        """-> (results, mods): `results` is exactly what `call` returns; mods[r] is a float32 array (len(sequence r),
        nmod): row i holds, for character i of read r's call, the log-probabilities of the modifications of ITS
        canonical base (the network's categorical columns at the block before the move, flipflopfings.py:100-143) and
        NaN in the columns of the other bases' modifications; columns in can_nmods order.  With reverse=True the rows
        are in the order of the unreversed call string in `results` -- the call of the reversed signal -- which
        `write_records(reverse=True)` writes back to front.  The network runs once per slice, and the scores ride in
        the call's one download, behind seq | qual."""
        if not self.can_nmods:
            raise RuntimeError("Basecaller.call_mods needs mod_output=True at construction")
        return self._call(signals, read_params, True)

    def _call(self, signals, read_params, want_mods):
        """-> (results, every read's modified-base scores or None); nothing waits on the host before the download."""
        if len(signals) == 0:
            return [], []
        sigs = [np.asarray(s, dtype=np.float32).reshape(-1) for s in signals]
        if self.reverse:
            sigs = [s[::-1] for s in sigs]
        params = list(read_params) if read_params is not None else [None] * len(sigs)
        with torch.cuda.device(self.device), torch.no_grad():
            c = self._upload(sigs, params)                                              # 1.
            self._normalisation(c, np.array([p is not None for p in params]))           # 2.
            counts = chunk_counts(c.lens, self.chunk_size, self.overlap)
            chunks, geo = self._chunk(c, int(counts.sum()))                             # 3.
            batch, short = self._network(c, self.plan(c.lens), chunks, geo, want_mods)  # 4.-8.
            rooms = [(s.r0 + i, n) for s in short for i, n in enumerate([s.nrow] if s.rooms is None else s.rooms)]
            grow = np.zeros(c.nvirt - c.nread, dtype=np.int64)       # (the batched short reads: no chunk of the batch's)
            off = room_offsets(np.concatenate([counts, grow]), np.concatenate([c.lens, grow]),
                               batch.nrow if batch else 0, rooms, self.chunk_size, self.overlap, self.stride)
            # Order is behaviour: the batch's launch comes first and writes a length of 0 for every read without a
            # chunk in it; the short reads follow in plan order, each over its own slot.
            segs = ([batch] if batch else []) + short
            layout, body = (self._decode_beam(c, segs, off) if self.beam                # 9.
                            else self._decode_viterbi(c, segs, off, want_mods))
            return self._download(c, layout, body, off, want_mods)                      # 10.

    def _upload(self, sigs, params):
        """Step 1, the ONE upload: signals | offsets | the caller's shift and scale -> the call's device state.  The
        ONE download starts with its `head`: seqlen | status (the decoders put seq | qual | mods behind it).
        batch_short: the reads shorter than a chunk, in read order, are numbered nread, nread + 1, ... as well (`nvirt`
        entries in all): under those numbers they have their rooms, call lengths and scales, contiguous per slice, which
        is what the tail's per-read arrays need; the upload carries their list, the download is mapped back."""
        nread, lens = len(sigs), np.array([len(s) for s in sigs], dtype=np.int64)
        nsig = int(lens.sum())
        short = np.flatnonzero((lens > 0) & (lens < self.chunk_size)).astype(np.int32) if self.batch_short else None
        nvirt = nread + (len(short) if self.batch_short else 0)
        up = _Layout([("signal", np.float32, nsig), ("sig_off", np.int64, nread + 1), ("shift", np.float32, nread),
                      ("scale", np.float32, nread)] + ([("short", np.int32, len(short))] if self.batch_short else []))
        host = np.zeros(_align(up.nbytes), dtype=np.uint8)
        up.view(host, "signal")[:] = np.concatenate(sigs) if nsig else 0
        up.view(host, "sig_off")[:] = np.concatenate([[0], np.cumsum(lens)])
        up.view(host, "shift")[:] = [p[0] if p is not None else 0 for p in params]
        up.view(host, "scale")[:] = [p[1] if p is not None else 1 for p in params]
        if self.batch_short:
            up.view(host, "short")[:] = short
        dev = torch.from_numpy(host).to(self.device)
        head_layout = _Layout([("seqlen", np.int32, nvirt), ("status", np.uint8, 16)])
        head = torch.zeros(head_layout.nbytes, dtype=torch.uint8, device=self.device)
        return types.SimpleNamespace(
            L=_lib.basecall_lib(), stream=_lib.stream_ptr(), nread=nread, lens=lens, nsig=nsig, nvirt=nvirt,
            short=short, short_dev=up.view(dev, "short") if self.batch_short else None,
            signal=up.view(dev, "signal", max(nsig, 1)), sig_off=up.view(dev, "sig_off"), shift=up.view(dev, "shift"),
            scale=up.view(dev, "scale"), head_layout=head_layout, head=head, seqlen=head_layout.view(head, "seqlen"),
            status=head_layout.view(head, "status"))

    def _normalisation(self, c, given):
        """Step 2: median / MAD where the caller gave no parameters, beside those it gave."""
        self._med_mad(c, given)
        if self.batch_short:        # the scales in the extended numbering (a refused read is refused under either number)
            c.scale = torch.cat([c.scale, c.scale.index_select(0, c.short_dev)])

    def _med_mad(self, c, given):
        if given.all():
            return
        medmad = torch.empty(2, c.nread, dtype=torch.float32, device=self.device)
        _lib.check(c.L.tk_signal_med_mad_dev(_lib.ptr(c.signal), _lib.ptr(c.sig_off), c.nread, _lib.ptr(medmad[0]),
                                             _lib.ptr(medmad[1]), _lib.ptr(c.status), c.stream),
                   "tk_signal_med_mad_dev")
        if given.any():
            mask = torch.from_numpy(given).to(self.device)
            c.shift, c.scale = torch.where(mask, c.shift, medmad[0]), torch.where(mask, c.scale, medmad[1])
        else:
            c.shift, c.scale = medmad[0], medmad[1]

    def _gather(self, c, r0, nread, overlap, chunks, geo, ws):
        """Normalise + chunk reads [r0, r0 + nread) into `chunks` (size, columns, 1); geo: starts, ends, offsets."""
        _lib.check(c.L.tk_basecall_gather_chunks_dev(
            _lib.ptr(c.signal), _at(c.sig_off, r0), nread, c.nsig, _at(c.shift, r0), _at(c.scale, r0), chunks.shape[0],
            overlap, chunks.shape[1], _lib.ptr(chunks), _lib.ptr(geo[0]), _lib.ptr(geo[1]), _lib.ptr(geo[2]),
            _lib.ptr(ws), ws.numel(), _lib.ptr(c.status), c.stream), "tk_basecall_gather_chunks_dev")

    def _chunk(self, c, total):
        """Step 3 for the reads of a chunk or more: the batch's chunk tensor and its starts, ends, read_chunk_off."""
        dev = self.device
        geo = [torch.empty(n, dtype=torch.int64, device=dev) for n in (max(total, 1), max(total, 1), c.nread + 1)]
        chunks = torch.empty(self.chunk_size, total, 1, dtype=torch.float32, device=dev)
        ws = torch.empty(max(c.L.tk_basecall_gather_workspace_bytes(total), 16), dtype=torch.uint8, device=dev)
        self._gather(c, 0, c.nread, self.overlap, chunks, geo, ws)
        return chunks, geo

    def _network(self, c, plan, chunks, geo, want_mods):
        """Steps 4-8 over the plan: the network on column slices of the batch's chunk tensor and on each short read as
        one chunk of its own length (step 3 for it), then the operators -> (the batch's segment or None, the short)."""
        dev, outs, short, k0 = self.device, [], [], 0
        one = torch.tensor([0, 1], dtype=torch.int64, device=dev)      # read_chunk_off of a read called alone
        for sl in plan:
            if not sl.short:
                outs.append(self.model(chunks[:, sl.first:sl.first + sl.ncol].contiguous()))
                continue
            if self.batch_short:
                short.append(self._short_slice(c, sl, k0, want_mods))
                k0 += sl.ncol
                continue
            own = torch.empty(int(c.lens[sl.first]), 1, 1, dtype=torch.float32, device=dev)
            own_geo = torch.empty(3, 2, dtype=torch.int64, device=dev)
            self._gather(c, sl.first, 1, 0, own, own_geo, torch.empty(16, dtype=torch.uint8, device=dev))
            short.append(Segment(sl.first, 1, 1, own_geo[0], own_geo[1], one,
                                 *self._operators([self.model(own)], want_mods)))
        batch = Segment(0, c.nread, chunks.shape[1], *geo, *self._operators(outs, want_mods)) if outs else None
        return batch, short

    def _short_slice(self, c, sl, k0, want_mods):
        """Steps 3-8 for a slice of short reads, the k0-th .. of the call's, as zero-padded columns: ONE gather, ONE
        network pass, the operators with the columns' lengths -> a Segment in the extended numbering.  Every column is
        a read of one chunk: starts 0, ends its length, and a path whose rows behind the length repeat the last state."""
        dev, lens = self.device, c.lens[list(sl.reads)]
        x = torch.empty(int(lens.max()), sl.ncol, 1, dtype=torch.float32, device=dev)
        samples = torch.empty(sl.ncol, dtype=torch.int32, device=dev)
        _lib.check(_lib.decode_varlen_lib().tk_basecall_gather_columns_dev(
            _lib.ptr(c.signal), _lib.ptr(c.sig_off), c.nread, c.nsig, _lib.ptr(c.shift), _lib.ptr(c.scale),
            _at(c.short_dev, k0), sl.ncol, x.shape[0], _lib.ptr(x), _lib.ptr(samples), _lib.ptr(c.status), c.stream),
            "tk_basecall_gather_columns_dev")
        out, out_lens = layers.forward_varlen(self.model, x, lens)
        rows = samples
        for stride in self._row_strides:
            rows = layers.conv_out_lengths(rows, stride)
        ops = self._operators([out], want_mods, rows)
        rooms = np.full(sl.ncol, ops[0], dtype=np.int64) if self.beam else np.asarray(out_lens, dtype=np.int64) + 1
        return Segment(c.nread + k0, sl.ncol, sl.ncol, torch.zeros(sl.ncol, dtype=torch.int64, device=dev),
                       samples.long(), torch.arange(sl.ncol + 1, dtype=torch.int64, device=dev), *ops, rooms, rows)

    def _operators(self, outs, want_mods, lengths=None):
        """Steps 5-8 on the network's outputs for one chunk tensor (categorical columns lie behind the scores):
        temperature, posterior, the Viterbi path and its error probabilities, or the scores for a beam -> a Segment's
        nrow, path, err, trans, weights.  `lengths`: the rows of every column of a padded tensor."""
        trans = torch.cat([o[:, :, :self.n_can_state] for o in outs], 1) * self.temperature
        if self.posterior:
            trans = (decode.flipflop_make_trans(trans, lengths=lengths) + 1e-8).log()
        if self.beam:
            return trans.shape[0], None, None, trans.contiguous(), None
        path = decode.flipflop_viterbi_path(trans, lengths=lengths)
        err = qscores.errprobs_from_trans(trans, path) if self.fastq else None
        weights = torch.cat([o[:, :, self.n_can_state:] for o in outs], 1).contiguous() if want_mods else None
        return path.shape[0], path, err, None, weights

    def _launch_call(self, c, seg, out_off, seq, qual):
        """The tail: stitch, collapse, quality characters of the segment's reads, each at its out_off."""
        _lib.check(c.L.tk_basecall_call_dev(
            _lib.ptr(seg.path), _lib.ptr(seg.err), seg.nrow - 1, seg.ncol, _lib.ptr(seg.starts), _lib.ptr(seg.ends),
            _lib.ptr(seg.read_chunk_off), _at(c.scale, seg.r0), seg.nread, self.stride, len(self.alphabet),
            self.alphabet, self.qscore_scale, self.qscore_offset, _at(out_off, seg.r0), _lib.ptr(seq), _lib.ptr(qual),
            _at(c.seqlen, seg.r0), _lib.ptr(c.status), c.stream), "tk_basecall_call_dev")

    def _launch_mods(self, c, seg, out_off, mods):
        """The modified-base scores at the tail's moves: the same walk, the same offsets, the same seqlen."""
        _lib.check(c.L.tk_basecall_mod_weights_dev(
            _lib.ptr(seg.path), _lib.ptr(seg.weights), seg.nrow - 1, seg.ncol, _lib.ptr(seg.starts), _lib.ptr(seg.ends),
            _lib.ptr(seg.read_chunk_off), _at(c.scale, seg.r0), seg.nread, self.stride, len(self.alphabet),
            (ctypes.c_int * len(self.can_nmods))(*self.can_nmods), _at(out_off, seg.r0), _lib.ptr(mods),
            _at(c.seqlen, seg.r0), _lib.ptr(c.status), c.stream), "tk_basecall_mod_weights_dev")

    def _launch_stitch(self, c, seg, row_off, packed, nrows):
        """The stitched scores of the segment's reads, each from row row_off of the packed buffer."""
        _lib.check(c.L.tk_basecall_stitch_scores_dev(
            _lib.ptr(seg.trans), seg.nrow, seg.ncol, seg.trans.shape[2], _lib.ptr(seg.starts), _lib.ptr(seg.ends),
            _lib.ptr(seg.read_chunk_off), _at(c.scale, seg.r0), seg.nread, self.stride, _at(row_off, seg.r0),
            packed.shape[0], _lib.ptr(packed), _at(nrows, seg.r0), _lib.ptr(c.status), c.stream),
            "tk_basecall_stitch_scores_dev")

    def _decode_viterbi(self, c, segs, off, want_mods):
        """Step 9 on the Viterbi paths: seq | qual | mods, read r's characters (and rows of scores) from off[r].  The
        mod launches read the seqlen of the tail's, so they follow all of them."""
        cap, nmod = max(int(off[-1]), 1), sum(self.can_nmods) if want_mods else 0
        layout = _Layout([("seq", np.uint8, cap), ("qual", np.uint8, cap), ("mods", np.float32, cap * nmod)])
        out_off = torch.from_numpy(off).to(self.device)
        body = torch.empty(layout.nbytes, dtype=torch.uint8, device=self.device)
        for seg in segs:
            self._launch_call(c, seg, out_off, layout.view(body, "seq"), layout.view(body, "qual"))
        for seg in segs if want_mods else ():
            self._launch_mods(c, seg, out_off, layout.view(body, "mods"))
        return layout, body

    def _decode_beam(self, c, segs, off):
        """Step 9 with a beam (bin/basecall.py:216-221 for every read): the stitched scores of every segment in ONE
        packed buffer, read r's rows from off[r], and ONE launch of the beam search, which also writes the calls."""
        row_off = torch.from_numpy(off).to(self.device)
        packed = torch.empty(int(off[-1]), self.n_can_state, dtype=torch.float32, device=self.device)
        nrows = torch.zeros(c.nvirt, dtype=torch.int32, device=self.device)
        for seg in segs:
            self._launch_stitch(c, seg, row_off, packed, nrows)
            if seg.rows is not None:        # padded columns: the search stops at every read's own last row
                own = nrows[seg.r0:seg.r0 + seg.nread]
                own.copy_(torch.minimum(own, seg.rows))
        seq = decodeutil.beamsearch_packed(packed, row_off, nrows, int(np.diff(off).max()), self.alphabet,
                                           self.beam.width, self.beam_cut, self.beam.guided, c.status, c.seqlen)[3]
        cap = max(int(off[-1]), 1)
        return _Layout([("seq", np.uint8, cap)]), seq[:cap]

    def _download(self, c, layout, body, off, want_mods):
        """Step 10, the ONE download: head | body -> (results, every read's modified-base scores or None)."""
        got = torch.cat([c.head, body]).cpu().numpy()
        bits = int(c.head_layout.view(got, "status").view(np.uint32)[0])
        if bits & _lib.BASECALL_DEFINES["TK_STATUS_CHUNK_PLAN"]:
            raise RuntimeError("basecall: the device's chunk plan disagrees with the host's (status %#x)" % bits)
        called, got = c.head_layout.view(got, "seqlen"), got[c.head.numel():]
        where = np.arange(c.nread)
        if self.batch_short:
            where[c.short] = c.nread + np.arange(len(c.short))      # the batched short reads: back to read order
        spans = [slice(int(off[v]), int(off[v]) + int(called[v])) for v in where]
        seq = [layout.view(got, "seq")[s].tobytes().decode("ascii") for s in spans]
        qual = [layout.view(got, "qual")[s].tobytes().decode("ascii") if self.fastq else None for s in spans]
        mods = layout.view(got, "mods").reshape(-1, sum(self.can_nmods)) if want_mods else None
        return list(zip(seq, qual, (int(n) for n in c.lens))), ([mods[s].copy() for s in spans] if want_mods else None)

def write_records(fh, ids, results, fastq, reverse=False):
    """The output loop of bin/basecall.py:280-291: one FASTA / FASTQ record per read with a non-empty call
    (`reverse`: sequence and qualities written back to front).  Returns (nbase, ncalled, nread, nsample)."""
    nbase = ncalled = nread = nsample = 0
    for read_id, (basecall, qstring, read_nsample) in zip(ids, results):
        if basecall is not None and len(basecall) > 0:
            fh.write("{}{}\n{}\n".format("@" if fastq else ">", read_id, basecall[::-1] if reverse else basecall))
            nbase += len(basecall)
            ncalled += 1
            if fastq:
                fh.write("+\n{}\n".format(qstring[::-1] if reverse else qstring))
        nread += 1
        nsample += read_nsample
    return nbase, ncalled, nread, nsample
