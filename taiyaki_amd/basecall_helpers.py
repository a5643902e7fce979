"""Chunking and chunk stitching around the decode kernels (``taiyaki/basecall_helpers.py``): the host-side
restatements, with the reference's names, signatures and results.  `taiyaki_amd.basecall.Basecaller` does the same
work for a batch of reads on the device."""
import numpy as np
import torch

_DEFAULT_CHUNK_SIZE = 1000
_DEFAULT_OVERLAP = 100


def chunk_bounds(siglen, chunk_size, overlap):
    """(chunk_starts, chunk_ends) of `chunk_read` for a signal of `siglen` samples: a closed form of the length."""
    if siglen < chunk_size:
        return np.array([0]), np.array([siglen])
    ends = np.arange(chunk_size, siglen, chunk_size - overlap, dtype=int)
    ends = np.concatenate([ends, [siglen]], 0)
    return ends - chunk_size, ends


def chunk_read(signal, chunk_size, overlap):
    """basecall_helpers.py:11-43: overlapping chunks of `chunk_size` samples, the last one flush with the end of the
    signal -> (chunks (chunk_size, nchunks, 1) f4, chunk_starts, chunk_ends).  A signal shorter than `chunk_size` is
    one chunk of its own length, returned as `signal[:, None, None]`."""
    if len(signal) < chunk_size:
        return signal[:, None, None], np.array([0]), np.array([len(signal)])
    chunk_starts, chunk_ends = chunk_bounds(len(signal), chunk_size, overlap)
    index = chunk_starts[None, :] + np.arange(chunk_size)[:, None]
    chunks = np.empty((chunk_size, len(chunk_ends), 1), dtype="f4")
    chunks[:, :, 0] = np.asarray(signal)[index]
    return chunks, chunk_starts, chunk_ends


def get_model_device(model):
    """helpers.py: the device of the model's first parameter."""
    return next(model.parameters()).device


def guess_model_stride(net, input_shape=(720, 1, 1)):
    """helpers.py:150-162: the stride of a network, from the length of its output on a test input."""
    with torch.no_grad():
        out = net(torch.zeros(input_shape).to(get_model_device(net)))
    return int(round(input_shape[0] / out.size()[0]))


def stitch_chunks(out, chunk_starts, chunk_ends, stride, path_stitching=False):
    """Join per-chunk network outputs / Viterbi paths / error probabilities of overlapping
    chunks: every overlap is cut at its midpoint.  `out` is (time, chunks, ...); returns
    (blocks, ...).  `path_stitching` shifts every cut by one (the path has one more row than
    the blocks; the caller of the reference passes False, basecall.py:222-231)."""
    nchunks = out.shape[1]
    if nchunks == 1:
        return out[:, 0]
    shift = 1 if path_stitching else 0
    pieces = []
    for i in range(nchunks):
        if i == 0:
            lo = chunk_starts[0] // stride
        else:
            lo = (chunk_ends[i - 1] - chunk_starts[i]) // (2 * stride) + shift
        if i == nchunks - 1:
            hi = (chunk_ends[i] - chunk_starts[i]) // stride + shift
        elif i == 0:
            hi = (chunk_ends[0] + chunk_starts[1]) // (2 * stride) + shift
        else:
            hi = (chunk_ends[i] + chunk_starts[i + 1] - 2 * chunk_starts[i]) // (2 * stride) + shift
        pieces.append(out[lo:hi, i])
    return torch.cat(pieces, 0)


def run_model(normed_signal, model, chunk_size=_DEFAULT_CHUNK_SIZE, overlap=_DEFAULT_OVERLAP, max_concur_chunks=None,
              return_numpy=True, return_tensor_on_device=True):
    """basecall_helpers.py:97-158 (the hook megalodon calls): chunk `normed_signal`, run `model` on the chunks, at most
    `max_concur_chunks` at a time, and stitch the outputs.  `chunk_size` and `overlap` are in blocks of the model's
    stride.  Returns a numpy array (`return_numpy`), else a tensor on the model's device or on the host."""
    device = get_model_device(model)
    stride = guess_model_stride(model)
    chunk_size *= stride
    overlap *= stride
    chunks, chunk_starts, chunk_ends = chunk_read(normed_signal, chunk_size, overlap)
    chunks = torch.tensor(chunks)
    with torch.no_grad():
        if max_concur_chunks is None:
            out = model(chunks.to(device)).cpu()
        else:
            out = torch.cat([model(some.to(device)).cpu() for some in torch.split(chunks, max_concur_chunks, 1)], 1)
        stitched = stitch_chunks(out, chunk_starts, chunk_ends, stride)
    if return_numpy:
        return stitched.numpy()
    return stitched.to(device) if return_tensor_on_device else stitched
