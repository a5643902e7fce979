"""How good a call is: unit-cost global alignment of calls against references on the device.

The reference's workflow aligns with an external aligner and reads `accuracy = (alnlen - NM) / alnlen` off the
alignment (misc/assess_alignment.py:83-137).  Here the alignment is include/taiyaki_amd_align.h: distance D the least
number of non-match columns, matches M the most match columns at that distance, columns = M + D, accuracy = M / columns.
One wavefront per pair, every pair of a batch in one launch; there is no CPU fallback."""
import collections

import numpy as np
import torch

from taiyaki_amd import _lib, decode, flipflopfings

MAX_LEN, REG_BAND, MAX_BAND, MAX_CALL, MAX_CALL_BAND = (
    _lib.ALIGN_DEFINES["TK_ALIGN_" + k] for k in ("MAX_LEN", "REG_BAND", "MAX_BAND", "MAX_CALL", "MAX_CALL_BAND"))

Alignment = collections.namedtuple("Alignment", "distance matches columns exact accuracy")
Alignment.__doc__ = """Per pair, on the device: int32 distance, matches, columns (= matches + distance) and exact (1
where distance and matches are those of the full sweep), float32 accuracy (matches / columns, NaN where columns is 0)."""

# what the last `align_pairs_exact` took: launches, and the largest max_distance it reached (None: every diagonal)
last_exact = {"rounds": 0, "max_distance": 0}


def _check(rc, what):
    if rc == _lib.DEFINES["TK_ERR_UNSUPPORTED"]:
        raise ValueError("%s: beyond the limits of include/taiyaki_amd_align.h (sequences of %d codes, bands of %d "
                         "diagonals, paths of %d states)" % (what, MAX_LEN, MAX_BAND, MAX_CALL))
    _lib.check(rc, what)


def _result(distance, matches, exact):
    columns = matches + distance
    return Alignment(distance, matches, columns, exact, matches.float() / columns.float())


def _host_codes(seq):
    if isinstance(seq, str):
        seq = seq.encode()
    if isinstance(seq, (bytes, bytearray)):
        return np.frombuffer(bytes(seq), dtype=np.uint8)
    arr = np.asarray(seq)
    if arr.ndim != 1 or (arr.size and (arr.dtype.kind not in "iu" or arr.min() < 0 or arr.max() > 255)):
        raise ValueError("align_pairs: a sequence is a string, bytes or a 1-d array of codes 0..255")
    return arr.astype(np.uint8)


def _is_device_form(x):
    return isinstance(x, (tuple, list)) and len(x) == 2 and torch.is_tensor(x[0]) and torch.is_tensor(x[1])


def _band_widths(m, n, t):
    """numpy: the diagonals swept per pair (0 where max_distance is below |n - m|); t < 0: all"""
    diff = np.abs(n - m)
    p = np.maximum(t - diff, 0) // 2
    banded = np.minimum(n, np.maximum(0, n - m) + p) - np.maximum(-m, np.minimum(0, n - m) - p) + 1
    return np.where(t < 0, m + n + 1, np.where(t < diff, 0, banded))


class _Pairs:
    """Packed pairs on the device: codes and offsets of both sides; the lengths on the host where the host has them."""

    def __init__(self, queries, refs, what):
        self.m = self.n = None
        if _is_device_form(queries) != _is_device_form(refs):
            raise ValueError("%s: queries and refs are both host sequences or both (codes, offsets) device tensors" % what)
        if _is_device_form(queries):
            (self.q, self.q_off), (self.r, self.r_off) = queries, refs
            for t in (self.q, self.q_off, self.r, self.r_off):
                _lib.require_gpu(t, what)
            if self.q.dtype != torch.uint8 or self.r.dtype != torch.uint8 or self.q_off.dtype != torch.int64 or \
                    self.r_off.dtype != torch.int64 or self.q_off.shape != self.r_off.shape or self.q_off.dim() != 1 or \
                    self.q_off.numel() == 0:
                raise ValueError("%s: device pairs are (uint8 codes, int64 offsets of npair + 1 entries) twice" % what)
            self.q, self.q_off, self.r, self.r_off = (t.contiguous() for t in (self.q, self.q_off, self.r, self.r_off))
            self.npair, self.device = self.q_off.numel() - 1, self.q.device
            return
        if len(queries) != len(refs):
            raise ValueError("%s: %d queries for %d references" % (what, len(queries), len(refs)))
        qs, rs = [_host_codes(s) for s in queries], [_host_codes(s) for s in refs]
        self.npair, self.device, self._host = len(qs), None, (qs, rs)
        self.m = np.array([len(s) for s in qs], dtype=np.int64)
        self.n = np.array([len(s) for s in rs], dtype=np.int64)
        if self.npair and max(self.m.max(), self.n.max()) > MAX_LEN:
            raise ValueError("%s: a sequence is longer than %d codes" % (what, MAX_LEN))

    def upload(self):
        """host pairs, once their lengths passed the checks: the ONE upload, q_off | r_off | query codes | reference codes"""
        if self.device is not None:
            return self
        qs, rs = self._host
        self.device = torch.device("cuda", torch.cuda.current_device())
        nq, nr = int(self.m.sum()), int(self.n.sum())
        host = np.zeros(16 * (self.npair + 1) + nq + nr, dtype=np.uint8)
        offs = host[:16 * (self.npair + 1)].view(np.int64)
        offs[:self.npair + 1] = np.concatenate([[0], np.cumsum(self.m)])
        offs[self.npair + 1:] = np.concatenate([[0], np.cumsum(self.n)])
        host[16 * (self.npair + 1):] = np.concatenate(qs + rs + [np.zeros(0, dtype=np.uint8)])
        dev = torch.from_numpy(host).to(self.device)
        doffs = dev[:16 * (self.npair + 1)].view(torch.int64)
        self.q_off, self.r_off = doffs[:self.npair + 1], doffs[self.npair + 1:]
        self.q = dev[16 * (self.npair + 1):16 * (self.npair + 1) + nq]
        self.r = dev[16 * (self.npair + 1) + nq:]
        return self

    def lengths(self):
        """host lengths (device pairs: one read of the offsets)"""
        if self.m is None:
            qo, ro = self.q_off.cpu().numpy(), self.r_off.cpu().numpy()
            self.m, self.n = np.maximum(np.diff(qo), 0), np.maximum(np.diff(ro), 0)
        return self.m, self.n

    def launch(self, out, max_distance, shared, band_cells, pairs=None, what="align_pairs"):
        """one launch: every pair, or the pairs `pairs` (int32 on the device) names; results land at the pair's index"""
        count = self.npair if pairs is None else pairs.numel()
        if count == 0:
            return
        with torch.cuda.device(self.device):
            _check(_lib.align_lib().tk_align_pairs_dev(
                _lib.ptr(self.q) if self.q.numel() else _lib.ptr(self.q_off), _lib.ptr(self.q_off),
                _lib.ptr(self.r) if self.r.numel() else _lib.ptr(self.r_off), _lib.ptr(self.r_off), count,
                _lib.ptr(pairs), _lib.ptr(max_distance), shared, band_cells, _lib.ptr(out[0]), _lib.ptr(out[1]),
                _lib.ptr(out[2]), _lib.stream_ptr()), "tk_align_pairs_dev")


def _empty_out(npair, device):
    return [torch.zeros(npair, dtype=torch.int32, device=device) for _ in range(3)]


def align_pairs(queries, refs, max_distance=None):
    """Align queries[k] against refs[k] for every k, in one launch.

    queries, refs   lists of str / bytes / 1-d integer arrays (codes 0..255; one upload for all of them), or each a pair
                    of device tensors (uint8 codes of all sequences packed, int64 offsets of npair + 1 entries)
    max_distance    None: every diagonal is swept.  An int, or one int per pair (a host sequence or an int32 device
                    tensor): the band of include/taiyaki_amd_align.h; `exact` says where it held the answer.
    Returns an `Alignment` of device tensors; nothing is read back.  Lengths the host can see are checked against the
    limits (ValueError); pairs that live on the device and exceed them are reported with exact 0, distance
    max(m, n) and matches 0, as the pairs whose max_distance is below their difference in length are."""
    pk = _Pairs(queries, refs, "align_pairs")
    shared, per_pair, host_t = -1, None, None
    if torch.is_tensor(max_distance) and max_distance.is_cuda:
        if max_distance.shape != (pk.npair,):
            raise ValueError("align_pairs: max_distance holds one entry per pair")
        per_pair = max_distance.to(torch.int32).contiguous()
    elif max_distance is not None and np.ndim(max_distance) == 0:
        shared = int(max_distance)
        if shared < 0:
            raise ValueError("align_pairs: max_distance is None or >= 0")
        host_t = np.full(pk.npair, shared, dtype=np.int64)
    elif max_distance is not None:
        host_t = np.asarray(max_distance.cpu() if torch.is_tensor(max_distance) else max_distance).astype(np.int64)
        if host_t.shape != (pk.npair,):
            raise ValueError("align_pairs: max_distance holds one entry per pair")
        per_pair = host_t.astype(np.int32)
    if pk.m is not None and (max_distance is None or host_t is not None):
        t = host_t if host_t is not None else np.full(pk.npair, -1, dtype=np.int64)
        widest = int(_band_widths(pk.m, pk.n, t).max()) if pk.npair else 0
        if widest > MAX_BAND:
            raise ValueError("align_pairs: a band of %d diagonals; the kernels hold %d (give a max_distance, or use "
                             "align_pairs_exact)" % (widest, MAX_BAND))
    else:       # lengths (or bands) on the device: the bound the host has
        pk.upload()
        widest = min(MAX_BAND, pk.q.numel() + pk.r.numel() + 1)
        if shared >= 0:
            widest = min(widest, shared + 1)
    pk.upload()
    if isinstance(per_pair, np.ndarray):
        per_pair = torch.from_numpy(per_pair).to(pk.device)
    out = _empty_out(pk.npair, pk.device)
    pk.launch(out, per_pair, shared, max(widest, 1))
    return _result(*out)


def align_pairs_exact(queries, refs, start=None):
    """`align_pairs` with a band that grows until it holds every pair's answer: the result is the full sweep's, `exact`
    all ones, at the cost of the band and not of the table -- what whole reads against their references need.

    start   the first max_distance, an int or one per pair; None: |n - m| + max(16, min(m, n) // 16), the difference in
            length (which every alignment pays) plus room for one error in sixteen codes.  It affects time only.
    Each round launches the pairs that are not exact yet with their max_distance doubled, and reads their `exact` words
    (one host read per round).  A pair whose band would pass the kernels' widest raises ValueError.
    `last_exact` holds the rounds taken and the largest max_distance reached."""
    pk = _Pairs(queries, refs, "align_pairs_exact")
    m, n = pk.lengths()
    if pk.npair and max(m.max(), n.max()) > MAX_LEN:
        raise ValueError("align_pairs_exact: a sequence is longer than %d codes" % MAX_LEN)
    pk.upload()
    out = _empty_out(pk.npair, pk.device)
    diff, longest = np.abs(n - m), np.maximum(m, n)
    t = diff + np.maximum(16, np.minimum(m, n) // 16) if start is None else np.maximum(
        np.broadcast_to(np.asarray(start, dtype=np.int64), m.shape), diff)
    pending = np.arange(pk.npair)
    rounds = reached = 0
    while len(pending):
        # a max_distance of max(m, n) or more holds every alignment: the band that crosses the whole table
        tp = np.where(t[pending] >= longest[pending], -1, t[pending])
        widest = int(_band_widths(m[pending], n[pending], tp).max())
        if widest > MAX_BAND:
            raise ValueError("align_pairs_exact: a pair needs a band of %d diagonals; the kernels hold %d"
                             % (widest, MAX_BAND))
        tfull = np.full(pk.npair, -1, dtype=np.int32)
        tfull[pending] = tp
        up = torch.from_numpy(np.concatenate([tfull, pending.astype(np.int32)])).to(pk.device)
        pk.launch(out, up[:pk.npair], -1, max(widest, 1), pairs=up[pk.npair:], what="align_pairs_exact")
        rounds, reached = rounds + 1, max(reached, int(t[pending].max()))
        done = out[2].cpu().numpy()[pending] != 0           # the round's host read
        pending = pending[~done]
        t[pending] = np.maximum(2 * t[pending], 1)
    last_exact.update(rounds=rounds, max_distance=reached)
    return _result(*out)


def call_alignment(outputs, seqs, seqlens, lengths=None):
    """The Viterbi call of every column of `outputs` against that column's labels: an `Alignment` on the device.

    outputs   (T, N, S) flip-flop scores on the device (a cat-mod model's: its first nstate columns)
    seqs, seqlens   the loss's labels: flip-flop codes concatenated, and their count per column (host or device)
    lengths   as for `decode.flipflop_viterbi_path`: blocks per column
    The existing Viterbi kernel gives the path; one launch of tk_align_calls_dev collapses each column's path in its
    wave (the called bases never reach memory) and sweeps every diagonal against seqs % nbase."""
    _lib.require_gpu(outputs, "call_accuracy")
    if outputs.dim() != 3:
        raise ValueError("call_accuracy: outputs is (T, N, S)")
    T, N, S = outputs.shape
    nbase = flipflopfings.nbase_flipflop(S)
    if T + 1 > MAX_CALL:
        raise ValueError("call_accuracy: %d blocks; the kernel collapses paths of up to %d states" % (T, MAX_CALL))
    dev = outputs.device
    lens = None if lengths is None else decode._column_lengths(lengths, T, N, "call_accuracy").to(dev)
    path = decode.flipflop_viterbi_path(outputs, lens)
    seqs_d = torch.as_tensor(seqs).to(device=dev, dtype=torch.int32, non_blocking=True).contiguous()
    seqlens = torch.as_tensor(seqlens)
    if seqlens.shape != (N,):
        raise ValueError("call_accuracy: seqlens holds one entry per column")
    if seqlens.is_cuda:
        longest = seqs_d.numel()
        seqlens_d = seqlens.to(torch.int32).contiguous()
        seq_off = torch.cat([torch.zeros(1, dtype=torch.int64, device=dev), torch.cumsum(seqlens_d.long().clamp(min=0), 0)])
    else:
        host = np.maximum(seqlens.numpy().astype(np.int64), 0)
        if int(host.sum()) > seqs_d.numel():
            raise ValueError("call_accuracy: sum(seqlens) exceeds len(seqs)")
        longest = int(host.max()) if N else 0
        both = torch.from_numpy(np.concatenate([[0], np.cumsum(host), host])).to(dev)      # the prefix and the counts: one upload
        seq_off, seqlens_d = both[:N + 1], both[N + 1:].to(torch.int32)
    widest = T + 1 + longest + 1
    if widest > MAX_CALL_BAND:
        if not seqlens.is_cuda:
            raise ValueError("call_accuracy: %d blocks against %d labels; the kernel sweeps %d diagonals"
                             % (T, longest, MAX_CALL_BAND))
        widest = MAX_CALL_BAND
    out = _empty_out(N, dev)
    with torch.cuda.device(dev):
        _check(_lib.align_lib().tk_align_calls_dev(
            _lib.ptr(path), _lib.ptr(lens), T, N, nbase, _lib.ptr(seqs_d), _lib.ptr(seq_off), _lib.ptr(seqlens_d),
            widest, _lib.ptr(out[0]), _lib.ptr(out[1]), _lib.ptr(out[2]), _lib.stream_ptr()), "tk_align_calls_dev")
    return _result(*out)


def call_accuracy(outputs, seqs, seqlens, lengths=None):
    """Per-column accuracy (float32 on the device) of the Viterbi call against the labels: `call_alignment`'s."""
    return call_alignment(outputs, seqs, seqlens, lengths).accuracy


def summary(accuracy, bin_width=0.01):
    """Host side, as misc/assess_alignment.py's summary reads its accuracies: mean, median, mode (the centre of the
    fullest bin of its histogram's width, 0.01) and the share above 0.9.  NaN entries (no columns) are left out."""
    acc = np.asarray(accuracy.detach().cpu() if torch.is_tensor(accuracy) else accuracy, dtype=np.float64).ravel()
    acc = acc[~np.isnan(acc)]
    if acc.size == 0:
        return dict(n=0, mean=float("nan"), median=float("nan"), mode=float("nan"), above_90=float("nan"))
    nbin = int(round(1.0 / bin_width))
    counts = np.bincount(np.minimum((acc / bin_width).astype(np.int64), nbin - 1), minlength=nbin)
    return dict(n=int(acc.size), mean=float(acc.mean()), median=float(np.median(acc)),
                mode=float((np.argmax(counts) + 0.5) * bin_width), above_90=float((acc > 0.9).mean()))
