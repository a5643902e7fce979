"""Drop-in for the remapping chain of ``taiyaki.prepare_mapping_funcs`` (``oneread_remap``,
prepare_mapping_funcs.py:24-108) for a batch of reads on the device: the remapping network on every whole read,
``flipflop_remap`` on its transition scores and ``SignalMapping.from_remapping_path(...).Ref_to_signal``.

The reference runs read by read at N = 1.  Here the reads of a batch, sorted by length, share launches of the network
(`layers.forward_varlen`: a column's rows are what the column gives run alone), their valid rows are packed on the
device into the buffer tk_flipflop_remap_dev takes, and one launch of it and one of
tk_remap_path_to_ref_to_signal_dev finish all of them.  One upload (signals, parameters, index tables), one download
(scores, paths, Ref_to_signal).  There is no CPU fallback for the pipeline: a model that is not on an AMD GPU raises.
"""
import collections

import numpy as np
import torch

from taiyaki_amd import _lib, flipflop_remap, layers

Launch = collections.namedtuple("Launch", "reads nblk")
Launch.__doc__ = """One network launch of the remap plan: `reads` (indices into the batch, by non-decreasing length) are
its columns, `nblk` = the longest of them = the rows of its padded input."""


def remap_plan(lengths, max_columns):
    """The network launches for reads of `lengths` samples, host arithmetic on lengths alone: reads sorted by length
    (ties in batch order), cut into launches of at most `max_columns` columns.  Every read appears once; a launch costs
    what its last (longest) read costs, so its neighbours in length are the cheapest company."""
    if max_columns < 1:
        raise ValueError("remap_plan: max_columns must be at least 1")
    lengths = np.asarray(lengths, dtype=np.int64).reshape(-1)
    order = np.argsort(lengths, kind="stable")
    return [Launch(tuple(int(r) for r in order[lo:lo + max_columns]), int(lengths[order[lo:lo + max_columns]].max()))
            for lo in range(0, len(order), max_columns)]


def model_stride(model):
    """helpers.guess_model_stride: the product of the strides of the model's Convolution layers."""
    return int(np.prod([layer.stride for layer in model if isinstance(layer, layers.Convolution)], dtype=np.int64))


def network_out_lengths(model, lengths):
    """Rows `model` returns for columns of `lengths` samples run alone (`layers.conv_out_lengths` through every
    Convolution)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    for layer in model:
        if isinstance(layer, layers.Convolution):
            lengths = layers.conv_out_lengths(lengths, layer.stride)
    return lengths


def _usable(signal, reference, params):
    """signal.py:72-95 and oneread_remap's early returns: the trimmed (start, length) of a read that can be remapped,
    None for one that cannot."""
    ts, te = params["trim_start"], params["trim_end"]
    if not reference or not (np.isfinite(params["shift"]) and np.isfinite(params["scale"])) or params["scale"] == 0:
        return None
    if ts < 0 or te < 0 or ts + te >= len(signal):
        return None
    return int(ts), int(len(signal) - ts - te)


class _Upload:
    """Host arrays laid end to end in one pinned byte buffer (16-byte aligned segments): one copy to the device."""

    def __init__(self):
        self._parts, self._size = [], 0

    def add(self, array, dtype):
        array = np.ascontiguousarray(array, dtype=dtype).reshape(-1)
        at = self._size
        self._parts.append((at, array))
        self._size = (at + max(array.nbytes, 1) + 15) // 16 * 16
        return at, array.size, torch.from_numpy(np.empty(0, dtype=dtype)).dtype

    def to(self, device):
        host = torch.empty(max(self._size, 16), dtype=torch.uint8, pin_memory=True)
        view = host.numpy()
        for at, array in self._parts:
            view[at:at + array.nbytes] = array.view(np.uint8)
        self._dev = host.to(device, non_blocking=True)
        return self

    def __getitem__(self, handle):
        at, n, dtype = handle
        return self._dev[at:at + n * dtype.itemsize].view(dtype)


def remap_batch(signals, references, model, read_params, alphabet=flipflop_remap.DEFAULT_ALPHABET, localpen=0.0,
                stride=None, max_columns=64):
    """``oneread_remap``'s chain for a batch of reads: -> [(score, path, ref_to_signal) or None] per read.

    signals: float32 currents, untrimmed; read_params[r]: dict with `trim_start`, `trim_end`, `shift`, `scale` (the
    reference's per-read parameters); references: strings over `alphabet`; model: the remapping network (a
    `layers.Serial` on the GPU); stride: the model's (None: the product of its Convolution strides).
    score and path (T + 1 entries, -1 in the start / end state) are `flipflop_remap`'s on the network's scores of the
    standardised trimmed signal, ref_to_signal (len(reference) + 1 int32) is
    ``SignalMapping.from_remapping_path(path, reference, stride, sig).Ref_to_signal``.  A read with an empty reference,
    no samples left after trimming or non-finite parameters gets None and does not disturb the others.

    Standardisation is float32, one operation at a time ((x - shift) / scale), on the device; reads sorted by length
    share network launches of at most `max_columns` columns (`remap_plan`)."""
    nread = len(signals)
    assert nread == len(references) == len(read_params)
    dev = next(model.parameters()).device
    _lib.require_gpu(next(model.parameters()), "remap_batch")
    if stride is None:
        stride = model_stride(model)
    sigs = [np.asarray(s, dtype=np.float32).reshape(-1) for s in signals]
    usable = [_usable(s, ref, p) for s, ref, p in zip(sigs, references, read_params)]
    good = [r for r in range(nread) if usable[r] is not None]
    if not good:
        return [None] * nread

    # host arithmetic: where everything lies
    sig_off = np.concatenate([[0], np.cumsum([len(s) for s in sigs])]).astype(np.int64)
    start = np.array([sig_off[r] + usable[r][0] if usable[r] else 0 for r in range(nread)], dtype=np.int64)
    nsample = np.array([usable[r][1] if usable[r] else 0 for r in range(nread)], dtype=np.int64)
    nrow = network_out_lengths(model, nsample)
    for r in good:
        if not set(references[r]) <= set(alphabet):
            raise ValueError("remap_batch: reference %d has letters outside the alphabet %r" % (r, alphabet))
    idx = [flipflop_remap.remap_indices(references[r], alphabet) for r in good]
    T, M = nrow[good], np.array([len(references[r]) for r in good], dtype=np.int64)
    row_off = np.concatenate([[0], np.cumsum(T)]).astype(np.int64)
    seq_off = np.concatenate([[0], np.cumsum(M)]).astype(np.int64)
    tb_off = np.concatenate([[0], np.cumsum(T * ((M + 63) // 64))]).astype(np.int64)
    path_off = row_off + np.arange(len(good) + 1)
    step_cat = np.concatenate([i[0] for i in idx]) if int(M.sum()) > len(good) else np.zeros(1, dtype=np.int64)

    up = _Upload()
    h_sig = up.add(np.concatenate(sigs), np.float32)
    h_shift = up.add([p["shift"] if u else 0.0 for p, u in zip(read_params, usable)], np.float32)
    h_scale = up.add([p["scale"] if u else 1.0 for p, u in zip(read_params, usable)], np.float32)
    h_count = up.add(np.diff(sig_off), np.int64)
    h_stay, h_step = up.add(np.concatenate([i[1] for i in idx]), np.int32), up.add(step_cat, np.int32)
    h_row, h_seq, h_tb = up.add(row_off, np.int64), up.add(seq_off, np.int64), up.add(tb_off[:-1], np.int64)
    h_pen = up.add(np.broadcast_to(np.asarray(localpen, dtype=np.float64), (nread,))[good], np.float64)
    h_path = up.add(path_off, np.int64)
    h_start = up.add([usable[r][0] for r in good], np.int64)
    h_len = up.add([len(sigs[r]) for r in good], np.int64)

    total, npath, nrts = int(row_off[-1]), int(path_off[-1]), int(seq_off[-1]) + len(good)
    L = _lib.lib()
    with torch.no_grad(), torch.cuda.device(dev):
        up.to(dev)
        # 1. standardise: float32, one operation at a time
        nsig = int(sig_off[-1])
        shift = torch.repeat_interleave(up[h_shift], up[h_count], output_size=nsig)
        scale = torch.repeat_interleave(up[h_scale], up[h_count], output_size=nsig)
        std = (up[h_sig] - shift) / scale
        # 2. - 4. the network per launch of the plan; its valid rows packed for the remap
        packed = None
        for launch in remap_plan(nsample[good], max_columns):          # (its reads: positions in `good`)
            cols = [good[k] for k in launch.reads]
            x = torch.zeros(launch.nblk, len(cols), 1, dtype=torch.float32, device=dev)
            for j, r in enumerate(cols):
                x[:nsample[r], j, 0] = std[start[r]:start[r] + nsample[r]]
            out, out_len = layers.forward_varlen(model, x, nsample[cols])
            assert np.array_equal(out_len, nrow[cols])
            if packed is None:
                packed = torch.empty(total, out.shape[2], dtype=torch.float32, device=dev)
            for j, k in enumerate(launch.reads):
                packed[row_off[k]:row_off[k + 1]] = out[:T[k], j]
        # 5. - 6. one remap launch, one Ref_to_signal launch, on the device paths
        result = torch.empty(8 * len(good) + 8 * npath + 4 * nrts, dtype=torch.uint8, device=dev)
        score_d = result[:8 * len(good)].view(torch.float64)
        path_d = result[8 * len(good):8 * (len(good) + npath)].view(torch.int64)
        rts_d = result[8 * (len(good) + npath):].view(torch.int32)
        tb_d = torch.empty(max(int(tb_off[-1]), 1), dtype=torch.int64, device=dev)
        rc = L.tk_flipflop_remap_dev(_lib.ptr(packed), _lib.ptr(up[h_row]), packed.shape[1], _lib.ptr(up[h_stay]),
                                     _lib.ptr(up[h_step]), _lib.ptr(up[h_seq]), _lib.ptr(up[h_pen]), len(good),
                                     int(M.max()), _lib.ptr(score_d), _lib.ptr(path_d), _lib.ptr(tb_d),
                                     _lib.ptr(up[h_tb]), _lib.stream_ptr())
        _lib.check(rc, "tk_flipflop_remap_dev")
        rc = L.tk_remap_path_to_ref_to_signal_dev(_lib.ptr(path_d), _lib.ptr(up[h_path]), _lib.ptr(up[h_seq]),
                                                  _lib.ptr(up[h_start]), _lib.ptr(up[h_len]), int(stride), len(good),
                                                  _lib.ptr(rts_d), _lib.stream_ptr())
        _lib.check(rc, "tk_remap_path_to_ref_to_signal_dev")
        # 7. one download
        got = result.cpu().numpy()
    score = got[:8 * len(good)].view(np.float64)
    path = got[8 * len(good):8 * (len(good) + npath)].view(np.int64)
    rts = got[8 * (len(good) + npath):].view(np.int32)
    results = [None] * nread
    for k, r in enumerate(good):
        results[r] = (float(score[k]), path[path_off[k]:path_off[k + 1]].copy(),
                      rts[seq_off[k] + k:seq_off[k + 1] + k + 1].copy())
    return results
