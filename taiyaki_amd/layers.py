"""Drop-in for the hot-path entry points of ``taiyaki.layers`` plus the layer stack
that feeds them.

* ``flipflop_logpartition`` (taiyaki/layers.py:1875-1890) runs the gfx950 HIP
  kernels (csrc/logz_kernels.hip) instead of cupy / the T-step torch loop.
* ``Convolution``, ``Lstm``, ``GruMod``, ``Reverse``, ``Serial``, ``GlobalNormFlipFlop``
  and ``GlobalNormFlipFlopCatMod`` restate the reference layers minimally on
  PyTorch-ROCm (Conv1d): by scope they STAY PyTorch modules
  (BASELINE.json north_star) and only produce the (T, N, S) score tensor.
  ``Lstm`` and ``GruMod`` keep their nn.LSTM / nn.GRU parameters, but on the GPU their
  recurrences run as the persistent HIP kernels of csrc/lstm_kernels.hip
  (`LstmRecurrence`; size 96: csrc/lstm_local.hip; size 512: the same kernels from
  libtaiyaki_amd_lstm_large.so, include/taiyaki_amd_lstm_large.h, USE_HIP_LSTM_LARGE) and csrc/gru_kernels.hip (`GruRecurrence`):
  one Function per cell, on the launch of the first library that admits the call, in the order that `_rnn_route`
  states.  A narrow
  ``Convolution`` with swish runs as the fused HIP kernels of csrc/conv_kernels.hip
  (`SmallConvolution`); the mGru models' first layer (1 -> size channels on the raw signal, tanh) as those of
  csrc/conv_signal.hip (`SignalConvolution`).
* ``forward_varlen`` runs a ``Serial`` on a batch whose columns have different lengths: every column's rows are what
  the column gives run alone (``Lstm`` / ``GruMod`` ``forward(x, reverse, lengths)`` on the forward-only launches of
  include/taiyaki_amd_rnn_varlen.h; under grad mode on the training pair of include/taiyaki_amd_rnn_varlen_train.h).
* A batch wider than one launch of a recurrence admits runs as slabs of columns, one admitted launch after the other
  (include/taiyaki_amd_rnn_wide.h; USE_HIP_RNN_WIDE).
"""
import ctypes

import numpy as np
import torch
from torch import nn

from taiyaki_amd import _lib, flipflopfings


# ---------------------------------------------------------------------------
# (B) log-partition operator
# ---------------------------------------------------------------------------
def _logz_launch(x, want_grad):
    _lib.require_gpu(x, "flipflop_logpartition")
    L = _lib.lib()
    sc = x.detach().float().contiguous()
    if sc.data_ptr() % 16 != 0:
        sc = sc.clone()
    T, N, S = sc.shape
    nbase = flipflopfings.nbase_flipflop(S)
    dev = sc.device
    with torch.cuda.device(dev):
        logz = torch.empty(N, dtype=torch.float32, device=dev)
        grad = torch.empty_like(sc) if want_grad else None
        wsb = L.tk_flipflop_logz_workspace_bytes(T, N, nbase)
        if wsb == 0:
            raise RuntimeError("flipflop_logpartition: nbase=%d is not built" % nbase)
        ws = _lib.workspace(wsb, dev, "logz")
        status = _lib.status_word(dev)
        rc = L.tk_flipflop_logz_dev(_lib.ptr(sc), T, N, nbase, _lib.ptr(logz), _lib.ptr(grad),
                                    _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr())
        _lib.check(rc, "tk_flipflop_logz_dev")
        _lib.finish(status)
    return logz, grad


class LogZ(torch.autograd.Function):
    """cupy_extensions/flipflop.py:338-354: logZ forward; backward =
    posterior transition probabilities * g[:, None]."""

    @staticmethod
    def forward(ctx, scores):
        logz, grad = _logz_launch(scores, ctx.needs_input_grad[0])
        if grad is not None:
            ctx.save_for_backward(grad)
        return logz

    @staticmethod
    def backward(ctx, g):
        trans, = ctx.saved_tensors
        return trans * g[:, None]


class LogZVarlen(torch.autograd.Function):
    """logZ of every column on its own rows, (N,): the posterior with lengths of include/taiyaki_amd_decode_varlen.h (one
    wave per column; `decode.flipflop_make_trans(..., lengths=)` is the same launch).  backward = the posterior transition
    probabilities * g[:, None], rows at or beyond a column's length exactly 0."""

    @staticmethod
    def forward(ctx, scores, lengths):
        from taiyaki_amd import decode
        V, sc, lens, nbase, wsb = decode._varlen_args(scores, lengths, "flipflop_logpartition")
        T, N, _ = sc.shape
        with torch.cuda.device(sc.device):
            trans = torch.empty_like(sc)
            logz = torch.empty(N, dtype=torch.float32, device=sc.device)
            ws = _lib.workspace(wsb, sc.device, "decode_varlen")
            status = _lib.status_word(sc.device)
            _lib.check(V.tk_flipflop_posterior_varlen_dev(_lib.ptr(sc), _lib.ptr(lens), T, N, nbase, _lib.ptr(trans),
                                                          _lib.ptr(logz), _lib.ptr(ws), wsb, _lib.ptr(status),
                                                          _lib.stream_ptr()), "tk_flipflop_posterior_varlen_dev")
            _lib.finish(status)
        if ctx.needs_input_grad[0]:
            ctx.save_for_backward(trans)
        return logz

    @staticmethod
    def backward(ctx, g):
        trans, = ctx.saved_tensors
        return trans * g[:, None], None


def flipflop_logpartition(x, _never_use_cupy=False, lengths=None):
    """layers.py:1875-1890: log-partition function for each batch element, (N,).  `lengths` (a host sequence or a device
    int tensor, one time length 0..T per column): logZ of x[:lengths[n], n] per column (log nbase at length 0),
    differentiable, the gradient rows beyond a column's length 0 -- for the loss assembled from its two operators."""
    del _never_use_cupy
    if lengths is not None:
        return LogZVarlen.apply(x, lengths)
    return LogZ.apply(x)


def log_partition_flipflop(scores):
    """layers.py:1277-1299, the reference's torch statement of the same quantity: (N, 1).  Here it
    is the same HIP operator (differentiable through `LogZ`), not a T-step loop."""
    return flipflop_logpartition(scores).unsqueeze(1)


def global_norm_flipflop(scores):
    """layers.py:1302-1313"""
    T = scores.shape[0]
    return scores - flipflop_logpartition(scores)[None, :, None] / np.float32(T)


# ---------------------------------------------------------------------------
# layer stack (stays PyTorch-ROCm)
# ---------------------------------------------------------------------------
def swish(x):
    return x * torch.sigmoid(x)


def linear(x):
    """activation.linear of the reference: the identity."""
    return x


def _orthonormal_(param):
    """layers.py:37-96 initialises matrix parameters orthonormally."""
    with torch.no_grad():
        flat = param.view(param.shape[0], -1)
        nn.init.orthogonal_(flat)


def _truncated_normal_(param, sd):
    """layers.py:99-114"""
    with torch.no_grad():
        nn.init.trunc_normal_(param, std=sd, a=-2 * sd, b=2 * sd)


# False: every Convolution with `use_gemm` runs unfold + GEMM, for comparisons against the HIP operator
USE_HIP_CONV = True
_CU_COUNT = {}


def _cu_count(dev):
    n = _CU_COUNT.get(dev.index)
    if n is None:
        n = _CU_COUNT[dev.index] = torch.cuda.get_device_properties(dev).multi_processor_count
    return n


def _aligned(t):
    """Contiguous and 16-byte aligned (the kernels load and store float4)."""
    t = t.contiguous()
    return t if t.data_ptr() % 16 == 0 else t.clone()


class SmallConvolution(torch.autograd.Function):
    """swish(conv1d(x) + b) of a narrow `Convolution` (stride 1; the shapes tk_conv1d_small_supported names) on the
    kernels of csrc/conv_kernels.hip: one forward launch writes y; the backward recomputes the pre-activation from x
    and the weights and gives dx (when wanted), dW and db in one launch plus the fixed-order sum of its partial
    slabs.  No GEMM, unfold copy or element-wise kernel."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        T, N, cin = x.shape
        cout, _, winlen = weight.shape
        dev = x.device
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        if ctx.needs_input_grad[0]:
            x = _aligned(x.detach())
        else:
            # the network's input: a captured train step reloads that buffer in place before every replay, which
            # autograd refuses for a saved tensor -- keep a copy (made inside the captured graph; 4 bytes a sample)
            x = x.detach().clone(memory_format=torch.contiguous_format)
        with torch.cuda.device(dev):
            y = torch.empty(T, N, cout, dtype=torch.float32, device=dev)
            rc = _lib.lib().tk_conv1d_small_forward_dev(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), T, N, cin, cout,
                                                        winlen, _cu_count(dev), _lib.ptr(y), _lib.stream_ptr())
        _lib.check(rc, "tk_conv1d_small_forward_dev")
        ctx.save_for_backward(x, weight, bias)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, weight, bias = ctx.saved_tensors
        T, N, cin = x.shape
        cout, _, winlen = weight.shape
        dev = x.device
        L = _lib.lib()
        dy = _aligned(dy)
        with torch.cuda.device(dev):
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            dw, db = torch.empty_like(weight), torch.empty_like(bias)
            if T * N == 0:
                return dx, dw.zero_(), db.zero_()
            wsb = L.tk_conv1d_small_workspace_bytes(T, N, cin, cout, winlen, _cu_count(dev))
            ws = _lib.workspace(wsb, dev, "conv")
            rc = L.tk_conv1d_small_backward_dev(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), T, N, cin,
                                                cout, winlen, _cu_count(dev), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                                _lib.ptr(ws), wsb, _lib.stream_ptr())
        _lib.check(rc, "tk_conv1d_small_backward_dev")
        return dx, dw, db


# False: the 16 -> Cout, window 19, stride 5 layer runs unfold + GEMM (exactly as with USE_HIP_CONV = False), for
# comparisons against the kernels of include/taiyaki_amd_conv_strided.h
USE_HIP_CONV_STRIDED = True
# The workspace handed to those calls: one size, allocated once per stream, for every shape whose weight gradient has
# one partial result per run, i.e. at most 8192 rows per run: 344 064 rows on 256 CUs, 3.4 x the models' 102 400.  The
# need is then the weights' images (1.9 MB at most) + (CUs / tiles) partial results: 14.4 MB at 256 channels and 15.0 MB at
# 384 on 256 CUs, 16.9 and 17.4 MB on 304 CUs.  Only a batch beyond those rows (its runs are cut into two or more partial
# results each) or a device beyond about 440 CUs needs more; the cached buffer then regrows to that call's size.
_CONV_STRIDED_WORKSPACE_BYTES = 24 << 20


class StridedConvolution(torch.autograd.Function):
    """swish(conv1d(x) + b) of the mLstm models' third layer (16 -> Cout channels, window 19, stride 5; the shapes
    tk_conv_strided_supported names) on the kernels of csrc/conv_strided.hip.  Forward: one GEMM whose rows are read
    straight from x writes z and y (`save` False, the caller under no_grad: y alone).  Backward: dz in one element-wise
    launch, dx (when wanted) as a gather GEMM over dz, dW and db as one split-K launch and the fixed-order sum of its
    partial results.  x and z are saved; no window matrix exists, forward or backward."""

    @staticmethod
    def _workspace(L, T, N, cout, dev):
        wsb = max(L.tk_conv_strided_workspace_bytes(T, N, cout, _cu_count(dev)), _CONV_STRIDED_WORKSPACE_BYTES)
        return _lib.workspace(wsb, dev, "conv_strided"), wsb

    @staticmethod
    def forward(ctx, x, weight, bias, save):
        T, N, _ = x.shape
        cout = weight.shape[0]
        dev = x.device
        L = _lib.conv_strided_lib()
        x = _aligned(x.detach())
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        with torch.cuda.device(dev):
            y = torch.empty((T + 4) // 5, N, cout, dtype=torch.float32, device=dev)
            z = torch.empty_like(y) if save else None
            ws, wsb = StridedConvolution._workspace(L, T, N, cout, dev)
            rc = L.tk_conv_strided_forward_dev(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), T, N, cout,
                                               _cu_count(dev), _lib.ptr(z), _lib.ptr(y), _lib.ptr(ws), wsb,
                                               _lib.stream_ptr())
        _lib.check(rc, "tk_conv_strided_forward_dev")
        if save:
            ctx.save_for_backward(x, z, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, z, weight = ctx.saved_tensors
        T, N, _ = x.shape
        cout = weight.shape[0]
        dev = x.device
        L = _lib.conv_strided_lib()
        dy = _aligned(dy)
        with torch.cuda.device(dev):
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            dw = torch.empty_like(weight)
            db = torch.empty(cout, dtype=torch.float32, device=dev)
            dz = torch.empty_like(z)
            ws, wsb = StridedConvolution._workspace(L, T, N, cout, dev)
            rc = L.tk_conv_strided_backward_dev(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(z), _lib.ptr(weight), T, N, cout,
                                                _cu_count(dev), _lib.ptr(dz), _lib.ptr(dx), _lib.ptr(dw), _lib.ptr(db),
                                                _lib.ptr(ws), wsb, _lib.stream_ptr())
        _lib.check(rc, "tk_conv_strided_backward_dev")
        return dx, dw, db, None


# False: the 16 -> Cout layer at the shapes `StridedConvolution` does not take (the fast and the RNA models') runs unfold
# + GEMM (exactly as with USE_HIP_CONV or USE_HIP_CONV_STRIDED = False), for comparisons against the kernels of
# include/taiyaki_amd_conv_window.h
USE_HIP_CONV_WINDOW = True
# HIP launches of `WindowConvolution` by pass
conv_window_calls = {"forward": 0, "backward": 0}
# The (size, winlen, stride) that take those kernels in grad mode: the configurations whose forward + backward was
# measured not behind the unfold + GEMM path at the trainer's shapes (tools/convbench.py --window;
# profiles/r45_conv_window.txt).  Under no_grad every shape tk_conv_window_supported names takes them: there a read's
# scores being a function of the read and the weights alone is the point, as for the output layer.
CONV_WINDOW_GRAD_SHAPES = frozenset(
    [(size, 19, 5) for size in (96, 128)]
    + [(size, 31, stride) for size in (96, 128, 192, 256, 384) for stride in (10, 12)])
# The workspace handed to those calls, as _CONV_STRIDED_WORKSPACE_BYTES: one size for every shape whose weight gradient
# has one partial result per run (at most 8192 rows per run); a larger need regrows the cached buffer
_CONV_WINDOW_WORKSPACE_BYTES = 24 << 20


class WindowConvolution(torch.autograd.Function):
    """swish(conv1d(x) + b) of the mLstm models' third layer at the fast and the RNA models' shapes (16 -> Cout channels,
    window 19 or 31, stride 5, 10 or 12; the shapes tk_conv_window_supported names) on the kernels of
    csrc/conv_strided.hip as libtaiyaki_amd_conv_window.so builds them.  The contract of `StridedConvolution`: one GEMM
    whose rows are read straight from x writes z and y (`save` False, the caller under no_grad: y alone); the backward
    writes dz in one element-wise launch, dx (when wanted) as a gather GEMM over dz, dW and db as one split-K launch and
    the fixed-order sum of its partial results.  x and z are saved; no window matrix exists, forward or backward."""

    @staticmethod
    def _workspace(L, T, N, cout, winlen, stride, dev):
        wsb = max(L.tk_conv_window_workspace_bytes(T, N, cout, winlen, stride, _cu_count(dev)),
                  _CONV_WINDOW_WORKSPACE_BYTES)
        return _lib.workspace(wsb, dev, "conv_window"), wsb

    @staticmethod
    def forward(ctx, x, weight, bias, save, stride):
        T, N, _ = x.shape
        cout, _, winlen = weight.shape
        dev = x.device
        ctx.stride = stride
        L = _lib.conv_window_lib()
        x = _aligned(x.detach())
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        with torch.cuda.device(dev):
            y = torch.empty(-(-T // stride), N, cout, dtype=torch.float32, device=dev)
            z = torch.empty_like(y) if save else None
            ws, wsb = WindowConvolution._workspace(L, T, N, cout, winlen, stride, dev)
            rc = L.tk_conv_window_forward_dev(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), T, N, cout, winlen, stride,
                                              _cu_count(dev), _lib.ptr(z), _lib.ptr(y), _lib.ptr(ws), wsb,
                                              _lib.stream_ptr())
        _lib.check(rc, "tk_conv_window_forward_dev")
        conv_window_calls["forward"] += 1
        if save:
            ctx.save_for_backward(x, z, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, z, weight = ctx.saved_tensors
        T, N, _ = x.shape
        cout, _, winlen = weight.shape
        stride = ctx.stride
        dev = x.device
        L = _lib.conv_window_lib()
        dy = _aligned(dy)
        with torch.cuda.device(dev):
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            dw = torch.empty_like(weight)
            db = torch.empty(cout, dtype=torch.float32, device=dev)
            dz = torch.empty_like(z)
            ws, wsb = WindowConvolution._workspace(L, T, N, cout, winlen, stride, dev)
            rc = L.tk_conv_window_backward_dev(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(z), _lib.ptr(weight), T, N, cout,
                                               winlen, stride, _cu_count(dev), _lib.ptr(dz), _lib.ptr(dx), _lib.ptr(dw),
                                               _lib.ptr(db), _lib.ptr(ws), wsb, _lib.stream_ptr())
        _lib.check(rc, "tk_conv_window_backward_dev")
        conv_window_calls["backward"] += 1
        return dx, dw, db, None, None


# False: the mGru models' first layer (1 -> Cout channels, window 19, tanh) runs unfold + GEMM (exactly as with
# USE_HIP_CONV = False), for comparisons against the kernels of include/taiyaki_amd_conv_signal.h
USE_HIP_CONV_SIGNAL = True
# HIP launches of `SignalConvolution` by pass
conv_signal_calls = {"forward": 0, "backward": 0}


def _stream_ptr(dev):
    """The device's current stream as the C ABI takes it, without building a `torch.cuda.Stream` (`_lib.stream_ptr`
    costs the host as much as the rest of a `SignalConvolution` call)."""
    return _lib._vp(torch._C._cuda_getCurrentRawStream(dev.index))


class SignalConvolution(torch.autograd.Function):
    """tanh(conv1d(x) + b) of the mGru models' first layer (1 -> Cout channels on the raw signal, window 19, stride
    1 ... 8; the shapes tk_conv_signal_supported names) on the kernels of csrc/conv_signal.hip.  Forward: one launch
    writes y.  Backward: dz = dy (1 - y^2) in registers, dW and db as one launch of partial results and their sum in a
    fixed order; no dx (the layer takes this path only where its input needs no gradient).  `save` (the caller under
    grad mode): y and a copy of x are saved; False: nothing is."""

    @staticmethod
    def forward(ctx, x, weight, bias, save, stride):
        T, N, _ = x.shape
        cout = weight.shape[0]
        dev = x.device
        ctx.stride = stride
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        if save:
            # the network's input: a captured train step reloads that buffer in place before every replay, which
            # autograd refuses for a saved tensor -- keep a copy (made inside the captured graph; 4 bytes a sample)
            x = x.detach().clone(memory_format=torch.contiguous_format)
        else:
            x = x.detach().contiguous()
        with torch.cuda.device(dev):
            y = torch.empty(-(-T // stride), N, cout, dtype=torch.float32, device=dev)
            if T * N:
                rc = _lib.conv_signal_lib().tk_conv_signal_forward_dev(
                    _lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), T, N, cout, stride, _cu_count(dev), _lib.ptr(y),
                    _stream_ptr(dev))
                _lib.check(rc, "tk_conv_signal_forward_dev")
                conv_signal_calls["forward"] += 1
        if save:
            ctx.save_for_backward(x, y)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, y = ctx.saved_tensors
        T, N, _ = x.shape
        cout, stride = y.shape[2], ctx.stride
        dev = x.device
        L = _lib.conv_signal_lib()
        dy = _aligned(dy)
        with torch.cuda.device(dev):
            dw = torch.empty(cout, 1, 19, dtype=torch.float32, device=dev)
            db = torch.empty(cout, dtype=torch.float32, device=dev)
            if T * N == 0:
                return None, dw.zero_(), db.zero_(), None, None
            wsb = L.tk_conv_signal_workspace_bytes(T, N, cout, stride, _cu_count(dev))
            # the partial results (16 MB at most on 256 CUs): a block of the caching allocator, which orders its reuse
            # on the stream and belongs to the graph's pool under capture -- the call is short enough on the GPU for
            # the host's side of it to show (tools/convbench.py --signal)
            ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
            rc = L.tk_conv_signal_backward_dev(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(y), T, N, cout, stride,
                                               _cu_count(dev), _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), wsb,
                                               _stream_ptr(dev))
        _lib.check(rc, "tk_conv_signal_backward_dev")
        conv_signal_calls["backward"] += 1
        return None, dw, db, None, None


class Convolution(nn.Module):
    """layers.py:744-850: TBF in/out, pad (winlen//2, (winlen-1)//2), then activation.

    Same parameters as the reference (`conv.weight` (size, insize, winlen), `conv.bias`),
    but evaluated as window-unfold + GEMM: MIOpen's choices for these skinny 1-D
    shapes (batch 128 x 4000 samples, 1->4->16->256 channels) fall back to naive
    direct/weight-gradient kernels that cost more than the whole LSTM stack, while
    the same contraction as a rocBLAS GEMM is a few hundred microseconds.  Set
    `use_gemm=False` for the plain nn.Conv1d evaluation (identical result).

    The GEMM library is in turn the wrong tool for the two narrow layers at the head of the
    model (1 -> 4 and 4 -> 16 channels on raw samples): their weight gradients are 4 x 5 and
    16 x 20 results over 512 000 rows, one macro tile on nine workgroups, 3 ms each.  With
    `use_gemm` set, a float32 CUDA input, swish and a shape `tk_conv1d_small_supported` names,
    the layer runs as the fused HIP operator `SmallConvolution` (USE_HIP_CONV = False: never).

    The wide layer behind them (16 -> 192, 256 or 384 channels, window 19, stride 5, swish) runs as `StridedConvolution` where
    `tk_conv_strided_supported` names the shape (USE_HIP_CONV or USE_HIP_CONV_STRIDED = False: never): its GEMMs
    read x through the window's address map, so the 124 MB window matrix of the unfold path is never written.
    The same layer at the fast and the RNA models' shapes (window 19 or 31, stride 5, 10 or 12, 96 channels or more)
    runs as `WindowConvolution` where `tk_conv_window_supported` names the shape (any of USE_HIP_CONV,
    USE_HIP_CONV_STRIDED, USE_HIP_CONV_WINDOW = False: never): under no_grad always, in grad mode for the
    configurations of CONV_WINDOW_GRAD_SHAPES.  Sizes below 96 and other windows or strides run unfold + GEMM.

    The mGru models' first layer (1 -> 32 ... 384 channels on the raw signal, window 19, stride 1 ... 8, tanh) runs as
    `SignalConvolution` where `tk_conv_signal_supported` names the shape and the input needs no gradient (USE_HIP_CONV
    or USE_HIP_CONV_SIGNAL = False: never): plain FMAs over a row's 19 taps in a fixed order, so a row has the same
    bits in any batch, and a weight gradient without a window matrix, a pre-activation tensor or atomics.
    """

    def __init__(self, insize, size, winlen, stride=1, fun=torch.tanh, use_gemm=True):
        super().__init__()
        self.winlen = winlen
        self.stride = stride
        self.use_gemm = use_gemm
        self.pad = nn.ConstantPad1d((winlen // 2, (winlen - 1) // 2), 0)
        self.conv = nn.Conv1d(insize, size, winlen, stride=stride)
        self.activation = fun
        _orthonormal_(self.conv.weight)
        _truncated_normal_(self.conv.bias, 0.5)

    def _hip_small(self, x):
        w = self.conv.weight
        return (USE_HIP_CONV and self.activation is swish and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32
                and w.is_cuda and w.dtype == torch.float32
                and bool(_lib.lib().tk_conv1d_small_supported(w.shape[1], w.shape[0], self.winlen, self.stride)))

    def _hip_strided(self, x):
        w = self.conv.weight
        if not (USE_HIP_CONV and USE_HIP_CONV_STRIDED and self.activation is swish and x.is_cuda and x.dim() == 3
                and x.dtype == torch.float32 and w.is_cuda and w.dtype == torch.float32):
            return False
        L = _lib.conv_strided_lib()
        return bool(L.tk_conv_strided_supported(w.shape[1], w.shape[0], self.winlen, self.stride)
                    and L.tk_conv_strided_workspace_bytes(x.shape[0], x.shape[1], w.shape[0], _cu_count(x.device)))

    def _hip_window(self, x):
        w = self.conv.weight
        if not (USE_HIP_CONV and USE_HIP_CONV_STRIDED and USE_HIP_CONV_WINDOW and self.activation is swish and x.is_cuda
                and x.dim() == 3 and x.dtype == torch.float32 and w.is_cuda and w.dtype == torch.float32):
            return False
        if torch.is_grad_enabled() and (w.shape[0], self.winlen, self.stride) not in CONV_WINDOW_GRAD_SHAPES:
            return False
        L = _lib.conv_window_lib()
        return bool(L.tk_conv_window_supported(w.shape[1], w.shape[0], self.winlen, self.stride)
                    and L.tk_conv_window_workspace_bytes(x.shape[0], x.shape[1], w.shape[0], self.winlen, self.stride,
                                                         _cu_count(x.device)))

    def _hip_signal(self, x):
        w = self.conv.weight
        if not (USE_HIP_CONV and USE_HIP_CONV_SIGNAL and self.activation is torch.tanh and x.is_cuda and x.dim() == 3
                and x.shape[2] == 1 and x.dtype == torch.float32 and w.is_cuda and w.dtype == torch.float32
                and self.conv.bias.is_cuda and self.conv.bias.dtype == torch.float32
                and not (torch.is_grad_enabled() and x.requires_grad)):
            return False
        L = _lib.conv_signal_lib()
        return bool(L.tk_conv_signal_supported(w.shape[1], w.shape[0], self.winlen, self.stride)
                    and L.tk_conv_signal_workspace_bytes(x.shape[0], x.shape[1], w.shape[0], self.stride,
                                                         _cu_count(x.device)))

    def forward(self, x):
        if not self.use_gemm:
            out = self.activation(self.conv(self.pad(x.permute(1, 2, 0))))
            return out.permute(2, 0, 1)
        if self._hip_small(x):
            return SmallConvolution.apply(x, self.conv.weight, self.conv.bias)
        if self._hip_strided(x):
            w, b = self.conv.weight, self.conv.bias
            save = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or b.requires_grad)
            return StridedConvolution.apply(x, w, b, save)
        if self._hip_window(x):
            w, b = self.conv.weight, self.conv.bias
            save = torch.is_grad_enabled() and (x.requires_grad or w.requires_grad or b.requires_grad)
            return WindowConvolution.apply(x, w, b, save, self.stride)
        if self._hip_signal(x):
            w, b = self.conv.weight, self.conv.bias
            save = torch.is_grad_enabled() and (w.requires_grad or b.requires_grad)
            return SignalConvolution.apply(x, w, b, save, self.stride)
        # x: (T, N, C) -> pad time -> windows (Tout, N, C, winlen) -> GEMM with (C*winlen, size)
        xp = nn.functional.pad(x, (0, 0, 0, 0, self.winlen // 2, (self.winlen - 1) // 2))
        win = xp.unfold(0, self.winlen, self.stride)            # (Tout, N, C, winlen) view
        tout, n = win.shape[0], win.shape[1]
        w = self.conv.weight.reshape(self.conv.weight.shape[0], -1)     # (size, C*winlen)
        out = torch.addmm(self.conv.bias, win.reshape(tout * n, -1), w.t())
        return self.activation(out.view(tout, n, -1))


class _Rnn(nn.Module):
    def __init__(self, cell):
        super().__init__()
        self.rnn = cell
        for name, param in self.rnn.named_parameters():
            if 'bias_hh' in name:       # layers.py:522-532: redundant bias frozen at zero
                param.requires_grad = False
                with torch.no_grad():
                    param.zero_()
            elif 'weight' in name:
                _orthonormal_(param)
            else:
                _truncated_normal_(param, 0.5)

    def forward(self, x, reverse=False, lengths=None):
        if lengths is not None:
            return _rnn_forward_varlen(self, x, reverse, lengths)
        route = _rnn_route(self, x, False, False)
        if route:
            # The LSTM has no launch without lengths that saves nothing, so its main row saves whatever the grad mode,
            # and its slabs of columns do as that row does; every other row saves only where something needs a gradient
            save = (isinstance(self.rnn, nn.LSTM) and route[0] in (False, "wide")) or _needs_grad(x, self)
            return _rnn_apply(self, x, reverse, *route, None, save)
        if reverse:
            return torch.flip(self.rnn(torch.flip(x, (0,)))[0], (0,))
        return self.rnn(x)[0]


# False: every Lstm runs nn.LSTM (MIOpen on the GPU), for comparisons against the HIP recurrence
USE_HIP_LSTM = True
# True: `Lstm` / `GruMod` `forward(x, reverse, lengths)` and `forward_varlen` are differentiable under grad mode (the
# training pair of include/taiyaki_amd_rnn_varlen_train.h where a HIP launch takes the tensors).  False, the default: such
# a call under grad mode raises, as it always has: a caller that trains through variable-length batches says so.
TRAIN_VARLEN = False
# HIP launches of `Lstm` / `GruMod` `forward(x, reverse, lengths)` by kind: "saved" wrote the activations for a backward
# pass (include/taiyaki_amd_rnn_varlen_train.h), "inference" saved nothing (include/taiyaki_amd_rnn_varlen.h)
rnn_varlen_calls = {"saved": 0, "inference": 0}
# True: a batch wider than one launch of a recurrence admits (hip_lstm_workspace_bytes / hip_gru_workspace_bytes or the
# query with lengths for the call returns 0 for its width alone) runs on the entries of include/taiyaki_amd_rnn_wide.h,
# as slabs of columns, one admitted launch after the other, wherever `hip_rnn_wide_workspace_bytes` is not 0.
# False: such a batch runs nn.LSTM / nn.GRU (with lengths: every column alone), as it did before there were slabs
USE_HIP_RNN_WIDE = True
# calls of `Lstm` / `GruMod` that went through include/taiyaki_amd_rnn_wide.h by kind, as rnn_varlen_calls counts: "saved"
# wrote the activations for a backward pass, "inference" saved nothing
rnn_wide_calls = {"saved": 0, "inference": 0}
# False: the parameter gradients of LstmRecurrence.backward are two GEMMs and a sum over dG (what they are wherever
# tk_lstm_weight_grad_workspace_bytes is 0), for comparisons against the fused kernel
USE_HIP_LSTM_WGRAD = True
# True: the input projection x W_ih^T + b in front of a recurrence and the input gradient dG W_ih behind it run as
# tk_rnn_input_proj_dev / tk_rnn_input_grad_dev (include/taiyaki_amd_rnn_proj.h) wherever tk_rnn_proj_workspace_bytes is
# not 0.  That rule is the library's (csrc/rnn_proj.hip, proj_admitted: the shapes at which the kernel was measured faster
# than rocBLAS, profiles/r31_lstmbench.txt, profiles/r31_grubench.txt): for the forward projection a function of the two
# widths only, never of the number of rows, so training, inference and the variable-length paths of a layer all take the
# same projection; the input gradient, which only training computes, also needs 64000 rows.
# False: torch.addmm / `@` (rocBLAS), for comparisons against the kernel
USE_HIP_RNN_PROJ = True
# The workspace handed to those calls: one size for every shape (the widest pair of widths the rule admits needs 3.4 MiB),
# so the cached buffer is allocated once per stream and never regrown or returned to the allocator in pieces
_RNN_PROJ_WORKSPACE_BYTES = 4 << 20


def _rnn_proj(a2, w_ih, bias, grad):
    """The input projection a2 (rows, I) . w_ih^T + bias (grad False) or the input gradient a2 (rows, G H) . w_ih (grad
    True) of a recurrent layer: the kernel of include/taiyaki_amd_rnn_proj.h where it runs, the rocBLAS GEMM otherwise."""
    rows, k = a2.shape
    nout = w_ih.shape[1] if grad else w_ih.shape[0]
    dev = a2.device
    if (USE_HIP_RNN_PROJ and a2.is_cuda and a2.dtype == torch.float32 and w_ih.dtype == torch.float32
            and a2.is_contiguous()):
        P = _lib.rnn_proj_lib()
        wsb = P.tk_rnn_proj_workspace_bytes(rows, k, nout, _cu_count(dev))
        if wsb:
            w = w_ih.contiguous()
            out = torch.empty(rows, nout, dtype=torch.float32, device=dev)
            wsb = max(wsb, _RNN_PROJ_WORKSPACE_BYTES)
            ws = _lib.workspace(wsb, dev, "rnn_proj")
            if grad:
                rc = P.tk_rnn_input_grad_dev(_lib.ptr(a2), _lib.ptr(w), rows, nout, k, _cu_count(dev), _lib.ptr(out),
                                             _lib.ptr(ws), wsb, _lib.stream_ptr())
            else:
                rc = P.tk_rnn_input_proj_dev(_lib.ptr(a2), _lib.ptr(w), _lib.ptr(bias.contiguous()), rows, k, nout,
                                             _cu_count(dev), _lib.ptr(out), _lib.ptr(ws), wsb, _lib.stream_ptr())
            _lib.check(rc, "tk_rnn_input_grad_dev" if grad else "tk_rnn_input_proj_dev")
            return out
    return a2 @ w_ih if grad else torch.addmm(bias, a2, w_ih.t())


def hip_lstm_workspace_bytes(rnn, x):
    """Workspace of the HIP recurrence for this layer and input, 0 where it does not run (CPU tensors, other
    dtypes, nn.LSTM options the kernels do not implement, sizes the launch geometry does not cover)."""
    if not _hip_lstm_takes(rnn, x):
        return 0
    return _lib.lib().tk_lstm_workspace_bytes(x.shape[1], rnn.hidden_size, _cu_count(x.device))


# True: an Lstm at hidden size 512, which the other recurrence libraries do not cover, runs on the entries of
# include/taiyaki_amd_lstm_large.h (every batch width, with or without lengths) wherever
# `hip_lstm_large_workspace_bytes` is not 0.  False: it runs nn.LSTM (with lengths: every column alone), as it did
# before there were such kernels, for comparisons against them
USE_HIP_LSTM_LARGE = True
# calls of `Lstm` that went through include/taiyaki_amd_lstm_large.h by kind, as rnn_varlen_calls counts: "saved" wrote
# the activations for a backward pass, "inference" handed the kernel NULL for them
lstm_large_calls = {"saved": 0, "inference": 0}


def hip_lstm_large_workspace_bytes(rnn, x):
    """Workspace of the entries of include/taiyaki_amd_lstm_large.h for this nn.LSTM and input: not 0 at every batch
    width where `_hip_lstm_takes` admits the layer and the library supports its size (512), 0 elsewhere: other sizes,
    empty tensors, what `_hip_lstm_takes` refuses, and USE_HIP_LSTM_LARGE = False."""
    if not (USE_HIP_LSTM_LARGE and isinstance(rnn, nn.LSTM) and _hip_lstm_takes(rnn, x) and x.shape[0] and x.shape[1]):
        return 0
    L = _lib.lstm_large_lib()
    if not L.tk_lstm_large_supported(rnn.hidden_size):
        return 0
    return L.tk_lstm_large_workspace_bytes(x.shape[1], rnn.hidden_size, _cu_count(x.device))


# False: an Lstm at a size that only the kernels of include/taiyaki_amd_lstm_local.h cover (96) runs nn.LSTM, with
# lengths every column alone, as it did before there were such kernels, for comparisons against them
USE_HIP_LSTM_LOCAL = True
# calls of `Lstm` that went through include/taiyaki_amd_lstm_local.h by kind, as rnn_varlen_calls counts: "saved" wrote
# the activations for a backward pass, "inference" handed the kernel NULL for them
lstm_local_calls = {"saved": 0, "inference": 0}


def hip_lstm_local_takes(rnn, x):
    """True where the recurrence of include/taiyaki_amd_lstm_local.h runs this nn.LSTM on this input: what
    `_hip_lstm_takes` admits, at a size one workgroup holds (`tk_lstm_local_supported`), with at least one step and one
    column.  It needs no workspace, so there is no size to ask for."""
    return bool(USE_HIP_LSTM_LOCAL and _hip_lstm_takes(rnn, x) and x.shape[0] and x.shape[1]
                and _lib.lstm_local_lib().tk_lstm_local_supported(rnn.hidden_size))


def _hip_lstm_takes(rnn, x):
    if not (USE_HIP_LSTM and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32
            and rnn.weight_hh_l0.is_cuda and rnn.weight_hh_l0.dtype == torch.float32):
        return False
    return not (rnn.num_layers != 1 or rnn.bidirectional or not rnn.bias or rnn.batch_first or rnn.proj_size)


def hip_rnn_wide_workspace_bytes(rnn, x):
    """Workspace of the entries of include/taiyaki_amd_rnn_wide.h for this nn.LSTM or nn.GRU and input: not 0 at every
    batch width where the HIP recurrence covers the layer and its size (what `hip_lstm_workspace_bytes` /
    `hip_gru_workspace_bytes` rule out apart from the width, under the same switches), 0 elsewhere and with
    USE_HIP_RNN_WIDE = False."""
    lstm = isinstance(rnn, nn.LSTM)
    if not (USE_HIP_RNN_WIDE and (_hip_lstm_takes(rnn, x) if lstm else _hip_gru_takes(rnn, x))):
        return 0
    kind = _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM" if lstm else "TK_RNN_KIND_GRU"]
    return _lib.rnn_wide_lib().tk_rnn_wide_workspace_bytes(kind, x.shape[1], rnn.hidden_size, _cu_count(x.device))


# What a recurrence launches, by (row: per-column lengths given, or "wide": a batch cut into slabs, or a size with a
# library of its own; activations saved), the row being what `_rnn_route` chooses: the
# library (its accessor in _lib), the forward and the backward entry ("%s": lstm / gru) and the workspace's tag (None:
# the cell's own).  The wide entries take the lengths (NULL: none) and all the forward's outputs (NULL: not saved).
_RNN_LAUNCHES = {
    (False, True): ("lib", "tk_%s_forward_dev", "tk_%s_backward_dev", None),
    (False, False): ("lib", "tk_%s_forward_dev", None, None),       # the GRU alone: NULL for the activations
    (True, True): ("varlen_train_lib", "tk_%s_forward_varlen_save_dev", "tk_%s_backward_varlen_dev",
                   "rnn_varlen_train"),
    (True, False): ("varlen_lib", "tk_%s_forward_varlen_dev", None, "rnn_varlen"),
    ("wide", True): ("rnn_wide_lib", "tk_%s_forward_wide_dev", "tk_%s_backward_wide_dev", "rnn_wide"),
    ("wide", False): ("rnn_wide_lib", "tk_%s_forward_wide_dev", None, "rnn_wide"),
    # hidden size 512 (include/taiyaki_amd_lstm_large.h): one pair of entries, the arguments of the wide ones
    ("large", True): ("lstm_large_lib", "tk_%s_large_forward_dev", "tk_%s_large_backward_dev", "lstm_large"),
    ("large", False): ("lstm_large_lib", "tk_%s_large_forward_dev", None, "lstm_large"),
    # hidden size 96 (include/taiyaki_amd_lstm_local.h): the arguments of the wide entries less the workspace, its size
    # and the status word (_RNN_BARE_ROWS), so the tag is never read
    ("local", True): ("lstm_local_lib", "tk_%s_local_forward_dev", "tk_%s_local_backward_dev", None),
    ("local", False): ("lstm_local_lib", "tk_%s_local_forward_dev", None, None),
}
# The rows whose entries take neither workspace, workspace size nor status word (csrc/lstm_local.hip: one workgroup owns
# every unit of its columns)
_RNN_BARE_ROWS = frozenset({"local"})
# The counter a call on a row moves, by "saved" / "inference"; the main row has none (the GRU: gru_forward_calls)
_RNN_CALLS = {True: rnn_varlen_calls, "wide": rnn_wide_calls, "local": lstm_local_calls, "large": lstm_large_calls}


def _rnn_route(layer, x, lengths_given, save):
    """Which launch runs the recurrence of `layer` (an `Lstm` or a `GruMod`) on x: (row of _RNN_LAUNCHES, workspace
    bytes) of the first candidate that admits the call, None where none does (nn.LSTM / nn.GRU; with lengths every
    column alone).  The order, for both cells, with and without lengths:
      1. the main library (`hip_lstm_workspace_bytes` / `hip_gru_workspace_bytes`, row False); with lengths the library
         with lengths in its place (row True): the training pair where `save`, the inference launch otherwise, neither
         asked on a tensor without steps or columns.  `save` is read for nothing else;
      2. slabs of columns ("wide"), not asked on a tensor without steps or columns;
      3. the LSTM alone: size 96 ("local"), which has no workspace (0 bytes), then
      4. size 512 ("large").
    Every query is looked up when it is asked and none is asked behind the first that admits, so a call costs the host
    no more than the queries in front of its row."""
    rnn = layer.rnn
    lstm = isinstance(rnn, nn.LSTM)
    full = x.dim() == 3 and x.shape[0] and x.shape[1]
    if not lengths_given:
        first = (False, hip_lstm_workspace_bytes if lstm else hip_gru_workspace_bytes, True)
    else:
        first = (True, hip_rnn_varlen_train_workspace_bytes if save else hip_rnn_varlen_workspace_bytes, full)
    for row, query, asked in (first, ("wide", hip_rnn_wide_workspace_bytes, full),
                              ("local", hip_lstm_local_takes, lstm), ("large", hip_lstm_large_workspace_bytes, lstm)):
        wsb = asked and query(rnn, x)
        if wsb:
            return row, 0 if row in _RNN_BARE_ROWS else wsb
    return None


def _rnn_apply(layer, x, reverse, row, wsb, lens, save):
    """The recurrence of `layer` on x through the launch that `_rnn_route` chose: the one place that spells the
    arguments of `LstmRecurrence` / `GruRecurrence`."""
    rnn = layer.rnn
    function = LstmRecurrence if isinstance(rnn, nn.LSTM) else GruRecurrence
    return function.apply(x, rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0, bool(reverse), row, wsb,
                          lens, save)


def _rnn_launch(cell, row, lens, save, backward, ins, shape, reverse, outs, wsb, dev):
    """One launch of a recurrence, checked: the entry of _RNN_LAUNCHES[row, save] on `ins` (the lengths behind them where
    the entry takes them), T, N, H, the direction and the CU count, `outs`, then the workspace, its size and the status
    word (all three or, on a row of _RNN_BARE_ROWS, none) and the stream."""
    libname, fwd, bwd, tag = _RNN_LAUNCHES[row, bool(save)]
    name = (bwd if backward else fwd) % cell
    checked = ()
    if row not in _RNN_BARE_ROWS:
        ws = _lib.workspace(wsb, dev, tag or cell)
        status = _lib.status_word(dev)
        checked = (_lib.ptr(ws), wsb, _lib.ptr(status))
    ptrs = [_lib.ptr(t) for t in ins + ((lens,) if row else ())]
    rc = getattr(getattr(_lib, libname)(), name)(*ptrs, *shape, int(reverse), _cu_count(dev),
                                                 *[_lib.ptr(t) for t in outs], *checked, _lib.stream_ptr())
    _lib.check(rc, name)
    if checked:
        _lib.finish(status)


class LstmRecurrence(torch.autograd.Function):
    """One nn.LSTM layer (h0 = c0 = 0) with its recurrence on the HIP kernels.  Forward: G_x = x W_ih^T + b_ih +
    b_hh as one GEMM, then tk_lstm_forward_dev.  Backward: tk_lstm_backward_dev gives dG (the gates'
    pre-activation gradient, T x N x 4H), the parameter and input gradients are GEMMs / a sum over it.
    `reverse` runs the recurrence from the last time step (layers.Reverse) on tensors in time order.
    `row` and `wsb` are what `_rnn_route` chose, the first library in its order that admits the call (a key of
    _RNN_LAUNCHES with `save`).  False: the entries above.  True, with `lens` (a device int32 tensor, one entry per
    column; column n has lens[n] steps): the launches of include/taiyaki_amd_rnn_varlen_train.h; y, the gates, c and dG
    are 0 at and beyond every length, so the input and parameter gradients are the same sums over the whole padded
    tensors; `save` False is the launch of include/taiyaki_amd_rnn_varlen.h: nothing but y is allocated or written, and
    the call cannot be differentiated.  "wide": the entries of include/taiyaki_amd_rnn_wide.h; "large": those of
    include/taiyaki_amd_lstm_large.h (size 512); "local": those of include/taiyaki_amd_lstm_local.h (size 96).  These
    three take `lens` or None and `save` either way (not `save`: NULL for the activations, which are neither allocated
    nor written), and admit every batch width."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, reverse, row, wsb, lens, save):
        if row is False and not save:
            raise RuntimeError("the LSTM has no launch without lengths that saves nothing")
        T, N, _ = x.shape
        H = w_hh.shape[1]
        dev = x.device
        x = x.contiguous()
        w_hh = w_hh.contiguous()
        if row in _RNN_CALLS:
            _RNN_CALLS[row]["saved" if save else "inference"] += 1
        gx = _rnn_proj(x.view(T * N, -1), w_ih, b_ih + b_hh, False)
        y = torch.empty(T, N, H, dtype=torch.float32, device=dev)
        gates = torch.empty(T, N, 4 * H, dtype=torch.float32, device=dev) if save else None
        cell = torch.empty(T, N, H, dtype=torch.float32, device=dev) if save else None
        _rnn_launch("lstm", row, lens, save, False, (gx, w_hh), (T, N, H), reverse,
                    (y,) if row is True and not save else (y, gates, cell), wsb, dev)
        if save:
            ctx.save_for_backward(x, w_ih, w_hh, y, gates, cell, lens)
        ctx.reverse, ctx.wsb, ctx.row = reverse, wsb, row
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_ih, w_hh, y, gates, cell, lens = ctx.saved_tensors
        T, N, I = x.shape
        H = w_hh.shape[1]
        # (the size-96 entries refuse a pointer that is not 16-byte aligned, and dy is the one tensor not allocated here)
        dy = _aligned(dy) if ctx.row == "local" else dy.contiguous()
        dg = torch.empty_like(gates)
        _rnn_launch("lstm", ctx.row, lens, True, True, (w_hh, gates, cell, dy), (T, N, H), ctx.reverse, (dg,), ctx.wsb,
                    x.device)
        return _lstm_grads_from_dgates(dg, x, w_ih, w_hh, y, ctx.reverse, ctx.needs_input_grad) + (None,) * 5


def _lstm_grads_from_dgates(dg, x, w_ih, w_hh, y, reverse, need):
    """(dx, dW_ih, dW_hh, db_ih, db_hh) of one LSTM layer from dG = dL/d(pre-activation) (T, N, 4H), its input x and
    its output y; need[0..4]: which of them are wanted.  With per-column lengths dG and y are 0 beyond every length, so
    the same sums over the whole padded tensors are the sums over every column's own steps (x finite in the padding)."""
    T, N, I = x.shape
    H = w_hh.shape[1]
    dev = x.device
    dg2 = dg.view(T * N, 4 * H)
    dx = _rnn_proj(dg2, w_ih, None, True).view(T, N, I) if need[0] else None
    if USE_HIP_LSTM_WGRAD and need[1] and need[2] and (need[3] or need[4]):
        # the three parameter gradients in one pass over dG: dG^T [x | y shifted by a step | 1]
        W = _lib.wgrad_lib()
        wgb = W.tk_lstm_weight_grad_workspace_bytes(T, N, H, I, _cu_count(dev))
        if wgb:
            dw_ih, dw_hh = torch.empty_like(w_ih, memory_format=torch.contiguous_format), torch.empty_like(w_hh)
            db = torch.empty(4 * H, dtype=torch.float32, device=dev)
            wws = _lib.workspace(wgb, dev, "lstm_wgrad")
            rc = W.tk_lstm_weight_grad_dev(_lib.ptr(dg), _lib.ptr(x), _lib.ptr(y), T, N, H, I, int(reverse),
                                           _cu_count(dev), _lib.ptr(dw_ih), _lib.ptr(dw_hh), _lib.ptr(db),
                                           _lib.ptr(wws), wgb, _lib.stream_ptr())
            _lib.check(rc, "tk_lstm_weight_grad_dev")
            return dx, dw_ih, dw_hh, db if need[3] else None, db if need[4] else None
    dw_ih = dg2.t() @ x.view(T * N, I) if need[1] else None
    dw_hh = None
    if need[2]:
        # dW_hh = sum over steps of dG_t^T h_prev, h_prev = the output of the recurrence's previous step
        if T > 1:
            dgs, hp = (dg[:-1], y[1:]) if reverse else (dg[1:], y[:-1])
            dw_hh = dgs.reshape(-1, 4 * H).t() @ hp.reshape(-1, H)
        else:
            dw_hh = torch.zeros_like(w_hh)
    db = dg2.sum(0) if (need[3] or need[4]) else None
    return dx, dw_ih, dw_hh, db if need[3] else None, db if need[4] else None


class Lstm(_Rnn):
    """layers.py:491-606 (wraps nn.LSTM, bias_hh frozen).  On the GPU the recurrence runs on the HIP kernels
    (`LstmRecurrence`) of the first library that `_rnn_route` finds to admit the call; nn.LSTM evaluates CPU tensors,
    sizes no kernel covers, and USE_HIP_LSTM = False."""

    def __init__(self, insize, size):
        super().__init__(nn.LSTM(insize, size))


# False: every GruMod runs nn.GRU (MIOpen on the GPU), for comparisons against the HIP recurrence
USE_HIP_GRU = True


def hip_gru_workspace_bytes(rnn, x):
    """Workspace of the HIP recurrence for this layer and input, 0 where it does not run (CPU tensors, other
    dtypes, nn.GRU options the kernels do not implement, sizes the launch geometry does not cover)."""
    if not _hip_gru_takes(rnn, x):
        return 0
    return _lib.lib().tk_gru_workspace_bytes(x.shape[1], rnn.hidden_size, _cu_count(x.device))


def _hip_gru_takes(rnn, x):
    if not (USE_HIP_GRU and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32
            and rnn.weight_hh_l0.is_cuda and rnn.weight_hh_l0.dtype == torch.float32):
        return False
    return not (rnn.num_layers != 1 or rnn.bidirectional or not rnn.bias or rnn.batch_first)


def _time_sum_tn(a, b, rows=2048):
    """sum over (t, n) of a[t, n, :, None] * b[t, n, None, :] for a (T, N, M) and b (T, N, P): a^T b over T N rows,
    as a batched GEMM over runs of about `rows` rows whose partial results are then summed over the runs.  One GEMM
    accumulates all T N products of an entry in float32 in a row (64 000 at bench.py --config 1's layer: 3.6e-6 of
    the largest entry against float64, where MIOpen's weight gradient is at 6e-7)."""
    T, N, M = a.shape
    P = b.shape[2]
    tc = max(1, rows // N)
    B = T // tc
    if B < 2:
        return a.reshape(T * N, M).t() @ b.reshape(T * N, P)
    main = B * tc
    out = torch.bmm(a[:main].reshape(B, tc * N, M).transpose(1, 2), b[:main].reshape(B, tc * N, P)).sum(0)
    if main < T:
        out.addmm_(a[main:].reshape(-1, M).t(), b[main:].reshape(-1, P))
    return out


# forward launches of GruRecurrence by kind: "saved" wrote the activations for a backward pass, "inference" handed
# the kernel NULL for them (what a test or a profile reads to see which path a call took)
gru_forward_calls = {"saved": 0, "inference": 0}


# False: the parameter gradients of GruRecurrence.backward are the batched GEMMs and sums of `_gru_grads_from_dgates`
# (what they are wherever tk_gru_weight_grad_workspace_bytes is 0), for comparisons against the fused kernel
USE_HIP_GRU_WGRAD = True
# calls of `_gru_grads_from_dgates` that wanted parameter gradients, by what computed them: tk_gru_weight_grad_dev or
# the GEMMs
gru_wgrad_calls = {"kernel": 0, "gemm": 0}


class GruRecurrence(torch.autograd.Function):
    """One nn.GRU layer (h0 = 0) with its recurrence on the HIP kernels.  Forward: G_x = x W_ih^T + b_ih as one
    GEMM, then tk_gru_forward_dev (b_hh goes to the kernel: its third slab sits inside the reset gate's product).
    `save` False (GruMod.forward: grad mode off, or nothing that requires a gradient) hands NULL for the activations:
    they are neither allocated nor written, and the call cannot be differentiated.  Backward: tk_gru_backward_dev gives
    dG = dL/dG_x (T x N x 3H) and dq; the hidden side's pre-activation gradient is dG with dq as its third slab,
    and the input gradient is a GEMM over dG, the parameter gradients one fused pass over the two
    (`_gru_grads_from_dgates`).  `reverse` runs the recurrence from the
    last time step (layers.Reverse) on tensors in time order.
    `lens` (a device int32 tensor, one entry per column): column n has lens[n] steps, and the launches are those of
    include/taiyaki_amd_rnn_varlen_train.h (`save`) or include/taiyaki_amd_rnn_varlen.h (not `save`).  y, the
    activations, q, dG and dq are 0 at and beyond every length, so the input and parameter gradients are the same sums
    over the whole padded tensors.  `row` and `wsb` are what `_rnn_route` chose, as for `LstmRecurrence`."""

    @staticmethod
    def forward(ctx, x, w_ih, w_hh, b_ih, b_hh, reverse, row, wsb, lens, save):
        T, N, _ = x.shape
        H = w_hh.shape[1]
        dev = x.device
        x = x.contiguous()
        w_hh, b_hh = w_hh.contiguous(), b_hh.contiguous()
        # (grad mode is off inside forward and ctx.needs_input_grad ignores it: the caller decides)
        train = bool(save)
        if row in _RNN_CALLS:
            _RNN_CALLS[row]["saved" if train else "inference"] += 1
        if lens is None or train:
            gru_forward_calls["saved" if train else "inference"] += 1
        gx = _rnn_proj(x.view(T * N, -1), w_ih, b_ih, False)
        y = torch.empty(T, N, H, dtype=torch.float32, device=dev)
        gates = torch.empty(T, N, 3 * H, dtype=torch.float32, device=dev) if train else None
        q = torch.empty(T, N, H, dtype=torch.float32, device=dev) if train else None
        _rnn_launch("gru", row, lens, train, False, (gx, w_hh, b_hh), (T, N, H), reverse,
                    (y,) if row is True and not train else (y, gates, q), wsb, dev)
        if train:
            ctx.save_for_backward(x, w_ih, w_hh, y, gates, q, lens)
        ctx.reverse, ctx.wsb, ctx.row = reverse, wsb, row
        return y

    @staticmethod
    def backward(ctx, dy):
        x, w_ih, w_hh, y, gates, q, lens = ctx.saved_tensors
        T, N, I = x.shape
        H = w_hh.shape[1]
        dy = dy.contiguous()
        dg = torch.empty_like(gates)
        dq = torch.empty_like(q)
        _rnn_launch("gru", ctx.row, lens, True, True, (w_hh, y, gates, q, dy), (T, N, H), ctx.reverse, (dg, dq), ctx.wsb,
                    x.device)
        return _gru_grads_from_dgates(dg, dq, x, w_ih, w_hh, y, ctx.reverse, ctx.needs_input_grad) + (None,) * 5


def _gru_grads_from_dgates(dg, dq, x, w_ih, w_hh, y, reverse, need):
    """(dx, dW_ih, dW_hh, db_ih, db_hh) of one GRU layer from dG = dL/dG_x (T, N, 3H) and dq (T, N, H), its input x and
    its output y; need[0..4]: which of them are wanted.  With per-column lengths dG, dq and y are 0 beyond every length,
    so the same sums over the whole padded tensors are the sums over every column's own steps (x finite in the padding).
    The parameter gradients are one call of tk_gru_weight_grad_dev (include/taiyaki_amd_gru_wgrad.h) where both weight
    gradients and a bias gradient are wanted, the tensors are float32 on the GPU and the call has a workspace at the
    shape -- at every shape it was measured at it is faster than the GEMMs below (profiles/r30_gru_wgrad.txt), so no
    shape is excluded here -- and the GEMMs, sums and cats below otherwise (USE_HIP_GRU_WGRAD = False: always)."""
    T, N, I = x.shape
    H = w_hh.shape[1]
    dg2 = dg.view(T * N, 3 * H)
    dx = _rnn_proj(dg2, w_ih, None, True).view(T, N, I) if need[0] else None
    if (USE_HIP_GRU_WGRAD and need[1] and need[2] and (need[3] or need[4]) and dg.is_cuda
            and all(t.dtype == torch.float32 for t in (dg, dq, x, y, w_ih, w_hh))):
        # the four parameter gradients in one pass: [dG | dq]^T [x | y shifted by a step | 1]
        dev = x.device
        W = _lib.gru_wgrad_lib()
        wgb = W.tk_gru_weight_grad_workspace_bytes(T, N, H, I, _cu_count(dev))
        if wgb:
            dg, dq, x, y = dg.contiguous(), dq.contiguous(), x.contiguous(), y.contiguous()
            dw_ih, dw_hh = torch.empty_like(w_ih, memory_format=torch.contiguous_format), torch.empty_like(w_hh)
            db_ih = torch.empty(3 * H, dtype=torch.float32, device=dev)
            db_hh = torch.empty(3 * H, dtype=torch.float32, device=dev) if need[4] else None
            wws = _lib.workspace(wgb, dev, "gru_wgrad")
            rc = W.tk_gru_weight_grad_dev(_lib.ptr(dg), _lib.ptr(dq), _lib.ptr(x), _lib.ptr(y), T, N, H, I,
                                          int(reverse), _cu_count(dev), _lib.ptr(dw_ih), _lib.ptr(dw_hh),
                                          _lib.ptr(db_ih), _lib.ptr(db_hh), _lib.ptr(wws), wgb, _lib.stream_ptr())
            _lib.check(rc, "tk_gru_weight_grad_dev")
            gru_wgrad_calls["kernel"] += 1
            return dx, dw_ih, dw_hh, db_ih if need[3] else None, db_hh
    if any(need[1:5]):
        gru_wgrad_calls["gemm"] += 1
    dw_ih = _time_sum_tn(dg, x) if need[1] else None
    dw_hh = None
    if need[2]:
        # dW_hh = sum over steps of [dr_pre, dz_pre, dq]_t^T h_prev, h_prev = the output of the recurrence's
        # previous step (0 at its first)
        if T > 1:
            sl, hp = (slice(0, T - 1), y[1:]) if reverse else (slice(1, T), y[:-1])
            dw_hh = torch.cat([_time_sum_tn(dg[sl][:, :, :2 * H], hp), _time_sum_tn(dq[sl], hp)])
        else:
            dw_hh = torch.zeros_like(w_hh)
    db_ih = dg2.sum(0) if (need[3] or need[4]) else None
    db_hh = torch.cat([db_ih[:2 * H], dq.view(T * N, H).sum(0)]) if need[4] else None
    return dx, dw_ih, dw_hh, db_ih if need[3] else None, db_hh


class GruMod(_Rnn):
    """layers.py:609-725 (wraps nn.GRU, bias_hh frozen).  On the GPU the recurrence runs on the HIP kernels
    (`GruRecurrence`) of the first library that `_rnn_route` finds to admit the call; nn.GRU evaluates CPU tensors, sizes
    the kernels do not cover, and USE_HIP_GRU = False."""

    def __init__(self, insize, size):
        super().__init__(nn.GRU(insize, size))


def _rnn_varlen_workspace_bytes(rnn, x, train):
    lstm = isinstance(rnn, nn.LSTM)
    if not (_hip_lstm_takes(rnn, x) if lstm else _hip_gru_takes(rnn, x)):
        return 0
    kind = _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM" if lstm else "TK_RNN_KIND_GRU"]
    query = (_lib.varlen_train_lib().tk_rnn_varlen_train_workspace_bytes if train
             else _lib.varlen_lib().tk_rnn_varlen_workspace_bytes)
    return query(kind, x.shape[1], rnn.hidden_size, _cu_count(x.device))


def hip_rnn_varlen_workspace_bytes(rnn, x):
    """Workspace of the forward-only launch with per-column lengths (include/taiyaki_amd_rnn_varlen.h) for this nn.LSTM
    or nn.GRU and input, 0 where it does not run: what `hip_lstm_workspace_bytes` / `hip_gru_workspace_bytes` rule
    out, under the same switches."""
    return _rnn_varlen_workspace_bytes(rnn, x, False)


def hip_rnn_varlen_train_workspace_bytes(rnn, x):
    """Workspace of the training pair with per-column lengths (include/taiyaki_amd_rnn_varlen_train.h) for this nn.LSTM
    or nn.GRU and input, 0 where it does not run: the rule of `hip_rnn_varlen_workspace_bytes`."""
    return _rnn_varlen_workspace_bytes(rnn, x, True)


def _needs_grad(x, module):
    return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in module.parameters()))


def _rnn_forward_varlen(layer, x, reverse, lengths):
    """`Lstm` / `GruMod` forward on a batch whose column n has lengths[n] steps: rows [0, lengths[n]) of column n are
    what `layer(x[:lengths[n], n:n + 1], reverse)` gives, the rows beyond are 0.  Where a HIP launch admits the
    tensors, `LstmRecurrence` / `GruRecurrence` with the lengths: under grad mode with something that requires a
    gradient they save the activations (x must be finite in the padding: the parameter gradients are sums over the
    whole padded tensors); otherwise it is one launch of tk_lstm_forward_varlen_dev / tk_gru_forward_varlen_dev, which
    saves nothing.  The libraries behind those two in the order of `_rnn_route` take the lengths as well.  Every column
    alone at its own length otherwise (differentiable like any other call of the layer).
    Under grad mode the call needs
    layers.TRAIN_VARLEN = True; without it it raises, as it did before there was a backward with lengths."""
    T, N, _ = x.shape
    train = _needs_grad(x, layer)
    if train and not TRAIN_VARLEN:
        raise RuntimeError("%s.forward with lengths is inference only unless layers.TRAIN_VARLEN is set: call it under "
                           "torch.no_grad(), or set layers.TRAIN_VARLEN = True to train through variable-length "
                           "batches" % type(layer).__name__)
    route = _rnn_route(layer, x, True, train)
    if not route:
        host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
        assert len(host) == N and (N == 0 or (host.min() >= 0 and host.max() <= T)), "lengths: one per column, 0..T"
        y = x.new_zeros(T, N, layer.rnn.hidden_size)
        for n, ln in enumerate(host):
            if ln:
                y[:ln, n:n + 1] = layer(x[:ln, n:n + 1], reverse=reverse)
        return y
    with torch.cuda.device(x.device):
        lens = torch.as_tensor(lengths).to(device=x.device, dtype=torch.int32).reshape(-1).clamp(0, T).contiguous()
        assert lens.numel() == N, "lengths: one per column"
        return _rnn_apply(layer, x, reverse, *route, lens, train)


class Reverse(nn.Module):
    """layers.py:117-153"""

    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, x, lengths=None):
        if lengths is not None:
            if not isinstance(self.layer, (Lstm, GruMod)):
                raise TypeError("Reverse(%s) takes no lengths" % type(self.layer).__name__)
            return self.layer(x, reverse=True, lengths=lengths)
        if isinstance(self.layer, (Lstm, GruMod)):
            return self.layer(x, reverse=True)      # (the HIP recurrences run backwards in time themselves)
        return torch.flip(self.layer(torch.flip(x, (0,))), (0,))


class Residual(nn.Module):
    """layers.py:156-186: x + layer(x)"""

    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, x):
        return x + self.layer(x)


class Serial(nn.Sequential):
    """layers.py:944-982"""

    def __init__(self, layers):
        super().__init__(*layers)


# False: `SquigglePredictor` runs its layers one by one (the per-layer path), for comparisons against the fused operator
USE_HIP_SQUIGGLE_NET = True
# Size 64 at more rows (P x N) than this runs per layer (None: no limit): see SquigglePredictor.  0: measured, the size-64 kernels (one workgroup
# per CU: 107 KB of LDS) are behind the per-layer path in the forward at every shape tried, 353 against 301 us at 1000 rows
# and 651 against 401 us at 30 000, and no better than level with it forward + backward (profiles/r37_squiggle_net.txt).
# The kernels stay built and tested (the tests lift this limit); the model does not take them.
SQUIGGLE_NET_64_MAX_ROWS = 0
# calls of the fused operator since the module was loaded (tests and tools read them)
SQUIGGLE_NET_LAUNCHES = {"forward": 0, "backward": 0}


def _pointer_array(tensors):
    return (_lib._vp * len(tensors))(*[t.data_ptr() for t in tensors])


class SquiggleNet(torch.autograd.Function):
    """The squiggle predictor network on the kernels of csrc/squiggle_net.hip (include/taiyaki_amd_squiggle_net.h):
    the forward is one launch (under no_grad it writes y alone; otherwise also the layers' tanh outputs), the backward
    one launch and the fixed-order sum of its partial results.  `params`: w_0, b_0, w_1, b_1, ... where the module
    keeps them."""

    @staticmethod
    def forward(ctx, x, lens, save, depth, *params):
        P, N, _ = x.shape
        size, winlen = params[0].shape[0], params[0].shape[2]
        dev = x.device
        L = _lib.squiggle_net_lib()
        if ctx.needs_input_grad[0] or not save:
            x = x.detach().contiguous()
        else:       # (the network's input: a captured step reloads that buffer in place -- see SmallConvolution)
            x = x.detach().clone(memory_format=torch.contiguous_format)
        params = [p.detach().contiguous() for p in params]
        with torch.cuda.device(dev):
            y = torch.empty(P, N, 3, dtype=torch.float32, device=dev)
            saved = torch.empty(depth + 1, P, N, size, dtype=torch.float32, device=dev) if save else None
            if P * N:
                rc = L.tk_squiggle_net_forward_dev(_lib.ptr(x), _pointer_array(params), _lib.ptr(lens), P, N, size, depth,
                                                   winlen, _cu_count(dev), _lib.ptr(saved), _lib.ptr(y),
                                                   _lib.stream_ptr())
                _lib.check(rc, "tk_squiggle_net_forward_dev")
                SQUIGGLE_NET_LAUNCHES["forward"] += 1
        if save:
            ctx.depth = depth
            ctx.save_for_backward(x, saved, lens, *params)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, saved, lens, *params = ctx.saved_tensors
        P, N, _ = x.shape
        size, winlen, depth = params[0].shape[0], params[0].shape[2], ctx.depth
        dev = x.device
        L = _lib.squiggle_net_lib()
        dy = dy.contiguous()
        with torch.cuda.device(dev):
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            grads = [torch.empty_like(p) for p in params]
            if P * N == 0:
                return (dx, None, None, None) + tuple(g.zero_() for g in grads)
            wsb = L.tk_squiggle_net_workspace_bytes(P, N, size, depth, winlen, _cu_count(dev))
            ws = _lib.workspace(wsb, dev, "squiggle_net")
            rc = L.tk_squiggle_net_backward_dev(_lib.ptr(dy), _lib.ptr(x), _lib.ptr(saved), _pointer_array(params),
                                                _lib.ptr(lens), P, N, size, depth, winlen, _cu_count(dev), _lib.ptr(dx),
                                                _pointer_array(grads), _lib.ptr(ws), wsb, _lib.stream_ptr())
            _lib.check(rc, "tk_squiggle_net_backward_dev")
            SQUIGGLE_NET_LAUNCHES["backward"] += 1
        return (dx, None, None, None) + tuple(grads)


class SquigglePredictor(Serial):
    """The network of bin/train_squiggle.py:86-94 (`models.squiggle_predictor`): a `Serial` of Convolution(3 -> size,
    tanh), `depth` Residual(Convolution(size -> size, tanh)) and Convolution(size -> 3, linear), every window the same.
    While its layers are exactly that pattern, the tensors are float32 on the GPU and `tk_squiggle_net_supported` and
    the workspace size say yes, the whole stack runs as the operator `SquiggleNet` (USE_HIP_SQUIGGLE_NET = False: never;
    size 64: only up to SQUIGGLE_NET_64_MAX_ROWS rows, which is none as measured); otherwise layer by layer, as any
    `Serial`.

    `lengths` (one value per column, at most the number of rows; a sequence, an array or a tensor): every layer's
    output of column n is zero at and beyond lengths[n], so the rows below it are what the column gives run alone."""

    def fused_shape(self):
        """(size, depth, winlen) if the layers are the pattern the kernels are written for, else None"""
        layers = list(self)
        if len(layers) < 3:
            return None
        first, last = layers[0], layers[-1]
        convs = [first] + [r.layer if type(r) is Residual else None for r in layers[1:-1]] + [last]
        if not all(type(c) is Convolution and c.stride == 1 and c.use_gemm for c in convs):
            return None
        size, winlen = first.conv.out_channels, first.winlen
        want = [(3, size, torch.tanh)] + [(size, size, torch.tanh)] * (len(layers) - 2) + [(size, 3, linear)]
        for c, (cin, cout, fun) in zip(convs, want):
            if (c.conv.in_channels, c.conv.out_channels, c.winlen) != (cin, cout, winlen) or c.activation is not fun \
                    or c.conv.bias is None:
                return None
        return size, len(layers) - 2, winlen

    def parameter_list(self):
        out = []
        for layer in self:
            conv = (layer.layer if type(layer) is Residual else layer).conv
            out += [conv.weight, conv.bias]
        return out

    def takes_operator(self, x):
        shape = self.fused_shape() if USE_HIP_SQUIGGLE_NET else None
        if shape is None or not (x.is_cuda and x.dim() == 3 and x.shape[2] == 3 and x.dtype == torch.float32):
            return False
        if not all(p.is_cuda and p.dtype == torch.float32 for p in self.parameter_list()):
            return False
        if shape[0] == 64 and SQUIGGLE_NET_64_MAX_ROWS is not None and x.shape[0] * x.shape[1] > SQUIGGLE_NET_64_MAX_ROWS:
            return False
        L = _lib.squiggle_net_lib()
        return bool(L.tk_squiggle_net_supported(*shape)) and (x.shape[0] * x.shape[1] == 0 or bool(
            L.tk_squiggle_net_workspace_bytes(x.shape[0], x.shape[1], *shape, _cu_count(x.device))))

    def _lengths(self, x, lengths):
        if lengths is None:
            return None
        if torch.is_tensor(lengths) and lengths.is_cuda:     # (device lengths: the kernels clamp them to the rows)
            lens = lengths
        else:
            host = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths).astype(np.int64)
            if host.shape != (x.shape[1],) or (host < 0).any() or (host > x.shape[0]).any():
                raise ValueError("SquigglePredictor: lengths must be one value in [0, %d] per column (%d columns)"
                                 % (x.shape[0], x.shape[1]))
            lens = torch.from_numpy(host)
        return lens.to(device=x.device, dtype=torch.int32).contiguous()

    def forward(self, x, lengths=None):
        lens = self._lengths(x, lengths)
        if self.takes_operator(x):
            params = self.parameter_list()
            save = torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in params))
            return SquiggleNet.apply(x, lens, save, len(self) - 2, *params)
        if lens is not None:        # (the input beyond a length counts as the padding it stands for; never in place)
            keep = torch.arange(x.shape[0], device=x.device)[:, None] < lens[None, :]
            x = x.masked_fill(~keep[:, :, None], 0)
        for layer in self:
            x = layer(x)
            if lens is not None:
                x = _zero_beyond(x, lens)
        return x


# False: the output layers run nn.Linear and the element-wise operators behind it, exactly as before the kernels of
# include/taiyaki_amd_out_layer.h, for comparisons against them
USE_HIP_OUT_LAYER = True
# Under no_grad the kernels take every supported shape: a row's scores then never depend on the rest of its batch.
# Under grad mode they take a layer from this many rows (T N) on, None: never -- where forward + backward was measured
# no slower than the library path (tools/outlayerbench.py, profiles/r44_out_layer.txt).  The cat-mod layer: 1.9 to 4.9 x
# faster at every shape measured (1600 to 102400 rows, three runs).  The plain layer: ahead or level at 1600 and 12800
# rows in most runs, but at 102400 rows 1.2 to 1.35 x slower at sizes 96 and 384 and between level and 1.3 x slower at
# 256; no number of rows from which it is ahead was found, so it keeps the library path under grad mode.
OUT_LAYER_GRAD_MIN_ROWS = 0
OUT_LAYER_PLAIN_GRAD_MIN_ROWS = None
# HIP launches of `OutLayer` by pass
out_layer_calls = {"forward": 0, "backward": 0}


def out_layer_tables(ntrans, can_nmods):
    """The cat-mod epilogue as include/taiyaki_amd_out_layer.h takes it: for every output column the linear column it
    reads (`src`) and -1 for 5 tanh or the base whose log_softmax group it belongs to (`group`).  The single canonical
    column `ntrans` opens every base's group, followed by that base's modifications."""
    src, group = list(range(ntrans)), [-1] * ntrans
    curr = 0
    for k, n in enumerate(can_nmods):
        src += [ntrans] + [ntrans + curr + 1 + i for i in range(int(n))]
        group += [k] * (1 + int(n))
        curr += int(n)
    return src, group


def _int_array(values):
    return (ctypes.c_int * len(values))(*values)


def hip_out_layer_takes(layer, x):
    """Whether `layer` (a GlobalNormFlipFlop or a GlobalNormFlipFlopCatMod) runs `x` on the kernels of
    include/taiyaki_amd_out_layer.h: the switch, a float32 CUDA tensor (T, N, I), a supported shape, and under grad
    mode at least OUT_LAYER_GRAD_MIN_ROWS (the plain layer: OUT_LAYER_PLAIN_GRAD_MIN_ROWS) rows."""
    w = layer.linear.weight
    if not (USE_HIP_OUT_LAYER and x.is_cuda and x.dim() == 3 and x.dtype == torch.float32 and w.is_cuda
            and w.dtype == torch.float32 and x.shape[2] == w.shape[1]):
        return False
    rows = x.shape[0] * x.shape[1]
    if rows == 0:
        return False
    if _needs_grad(x, layer):
        least = OUT_LAYER_GRAD_MIN_ROWS if isinstance(layer, GlobalNormFlipFlopCatMod) else OUT_LAYER_PLAIN_GRAD_MIN_ROWS
        if least is None or rows < least:
            return False
    L = _lib.out_layer_lib()
    nout = layer.nout if isinstance(layer, GlobalNormFlipFlopCatMod) else layer.size
    return bool(L.tk_out_layer_supported(w.shape[1], w.shape[0], nout)
                and L.tk_out_layer_workspace_bytes(rows, w.shape[1], w.shape[0], _cu_count(x.device)))


class OutLayer(torch.autograd.Function):
    """An output layer on the kernels of csrc/out_layer.hip.  Forward: one launch writes the weights' bf16 parts, one
    GEMM writes y finished (bias, scale tanh and the log_softmax groups in its epilogue; no pre-activation tensor).
    Backward: dz from dy and y alone, dx as a GEMM over it, dW and db as one launch over runs of rows and the
    fixed-order sum of its partial results.  y, x and w are saved and nothing else; `tables` is None (the plain layer)
    or the (src, group) int arrays of the cat-mod epilogue."""

    @staticmethod
    def forward(ctx, x, weight, bias, scale, nout, tables):
        T, N, I = x.shape
        dev = x.device
        L = _lib.out_layer_lib()
        x = x.detach().contiguous()
        weight, bias = weight.detach().contiguous(), bias.detach().contiguous()
        src, group = tables if tables is not None else (None, None)
        ctx.scale, ctx.tables = scale, tables
        with torch.cuda.device(dev):
            y = torch.empty(T, N, nout, dtype=torch.float32, device=dev)
            wsb = L.tk_out_layer_workspace_bytes(T * N, I, weight.shape[0], _cu_count(dev))
            ws = _lib.workspace(wsb, dev, "out_layer")
            rc = L.tk_out_layer_forward_dev(_lib.ptr(x), _lib.ptr(weight), _lib.ptr(bias), src, group, T * N, I,
                                            weight.shape[0], nout, scale, _cu_count(dev), _lib.ptr(y), _lib.ptr(ws),
                                            wsb, _stream_ptr(dev))
        _lib.check(rc, "tk_out_layer_forward_dev")
        out_layer_calls["forward"] += 1
        ctx.save_for_backward(y, x, weight)
        return y

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        y, x, weight = ctx.saved_tensors
        T, N, I = x.shape
        nlin, nout = weight.shape[0], y.shape[2]
        dev = x.device
        L = _lib.out_layer_lib()
        dy = dy.contiguous()
        src, group = ctx.tables if ctx.tables is not None else (None, None)
        with torch.cuda.device(dev):
            dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
            dw = torch.empty_like(weight)
            db = torch.empty(nlin, dtype=torch.float32, device=dev)
            wsb = L.tk_out_layer_workspace_bytes(T * N, I, nlin, _cu_count(dev))
            ws = _lib.workspace(wsb, dev, "out_layer")
            rc = L.tk_out_layer_backward_dev(_lib.ptr(dy), _lib.ptr(y), _lib.ptr(x), _lib.ptr(weight), src, group,
                                             T * N, I, nlin, nout, ctx.scale, _cu_count(dev), _lib.ptr(dx),
                                             _lib.ptr(dw), _lib.ptr(db), _lib.ptr(ws), wsb, _stream_ptr(dev))
        _lib.check(rc, "tk_out_layer_backward_dev")
        out_layer_calls["backward"] += 1
        return dx, dw, db, None, None, None


class GlobalNormFlipFlop(nn.Module):
    """layers.py:1316-1411: scale * tanh(x W + b); NO normalisation inside the layer."""

    def __init__(self, insize, nbase, scale=5.0):
        super().__init__()
        self.nbase = nbase
        self.size = flipflopfings.nstate_flipflop(nbase)
        self.linear = nn.Linear(insize, self.size)
        self.scale = scale
        _orthonormal_(self.linear.weight)
        _truncated_normal_(self.linear.bias, 0.5)

    def forward(self, x):
        if hip_out_layer_takes(self, x):
            return OutLayer.apply(x, self.linear.weight, self.linear.bias, float(self.scale), self.size, None)
        return self.scale * torch.tanh(self.linear(x))


class GlobalNormFlipFlopCatMod(nn.Module):
    """layers.py:1414-1640 for a canonical alphabet plus per-base modifications:
    output = [5 tanh(40 transition scores), per-base log_softmax over
    {canonical, its mods}] in the order A,(A mods),C,(C mods),...
    `can_nmods` = number of modified bases per canonical base."""

    def __init__(self, insize, can_nmods=(1, 1, 0, 0)):
        super().__init__()
        self.can_nmods = np.asarray(can_nmods)
        self.ncan_base = len(can_nmods)
        self.nmod_base = int(self.can_nmods.sum())
        self.ntrans_states = flipflopfings.nstate_flipflop(self.ncan_base)
        # layers.py:1495-1506
        self.can_mods_offsets = np.cumsum(
            np.concatenate([[0], self.can_nmods + 1])).astype(np.int32)
        self.can_indices = []
        curr = 0
        for n in self.can_nmods:
            self.can_indices.append(np.concatenate([[0], np.arange(curr + 1, curr + 1 + n)]))
            curr += n
        self.size = self.ntrans_states + 1 + self.nmod_base
        # index tensors live with the module (moved by .to(device)): nothing is uploaded in
        # forward, so the layer can be captured into a hipGraph
        for k, idx in enumerate(self.can_indices):
            self.register_buffer("can_index_%d" % k, torch.as_tensor(idx, dtype=torch.int64), persistent=False)
        self.linear = nn.Linear(insize, self.size)
        _orthonormal_(self.linear.weight)
        _truncated_normal_(self.linear.bias, 0.5)
        # the same epilogue as the kernels take it (host arrays: they travel in the launch's arguments)
        self.out_src, self.out_group = out_layer_tables(self.ntrans_states, self.can_nmods)

    @property
    def nout(self):
        return self.ntrans_states + self.ncan_base + self.nmod_base

    def forward(self, x):
        if hip_out_layer_takes(self, x):
            return OutLayer.apply(x, self.linear.weight, self.linear.bias, 5.0, self.nout,
                                  (_int_array(self.out_src), _int_array(self.out_group)))
        y = self.linear(x)
        trans = 5.0 * torch.tanh(y[:, :, :self.ntrans_states])
        cat = y[:, :, self.ntrans_states:]
        mods = [torch.log_softmax(cat.index_select(2, getattr(self, "can_index_%d" % k)), dim=2)
                for k in range(self.ncan_base)]
        return torch.cat([trans] + mods, dim=2)


def is_cat_mod_model(net):
    """layers.py:1643-1656: is the final layer of the `Serial` network a categorical modified-base layer?"""
    assert isinstance(net, Serial)
    return isinstance(net[-1], GlobalNormFlipFlopCatMod)


# ---------------------------------------------------------------------------
# a network pass on columns of different lengths
# ---------------------------------------------------------------------------
def conv_out_lengths(lengths, stride):
    """Rows a `Convolution` of this stride returns for a column of `lengths` samples run alone: ceil(length / stride),
    whatever the window (the layer pads winlen // 2 in front and (winlen - 1) // 2 behind); 0 stays 0.  Integers,
    arrays and tensors alike."""
    return (lengths + (stride - 1)) // stride


def _zero_beyond(y, lens_dev):
    """Rows t >= lens[n] of column n of y (T, N, C) set to 0: in place, or, under grad mode, in a new tensor (autograd
    may have saved y: tanh's output is its own saved tensor)."""
    keep = torch.arange(y.shape[0], device=y.device)[:, None] < lens_dev[None, :]
    if torch.is_grad_enabled():
        return y.masked_fill(~keep[:, :, None], 0)
    return y.masked_fill_(~keep[:, :, None], 0)


def _varlen_layers(model):
    """(layer, recurrent layer or None, reverse) for every layer of the Serial; TypeError for a type the pass does
    not know."""
    plan = []
    for layer in model:
        inner, rev = (layer.layer, True) if isinstance(layer, Reverse) else (layer, False)
        if isinstance(inner, (Lstm, GruMod)):
            plan.append((layer, inner, rev))
        elif not rev and isinstance(layer, (Convolution, GlobalNormFlipFlop, GlobalNormFlipFlopCatMod)):
            plan.append((layer, None, False))
        else:
            raise TypeError("forward_varlen: no rule for a layer of type %s" % (
                "Reverse(%s)" % type(inner).__name__ if rev else type(layer).__name__))
    return plan


def _varlen_batched(plan, x, lens):
    """The whole batch through every layer once; None where a recurrent layer has no HIP launch for its input."""
    h, lens_dev = x, torch.from_numpy(lens).to(x.device)
    if torch.is_grad_enabled():
        # the rows of x beyond a column's length belong to no column: their gradient is 0, whatever a window reads
        h = _zero_beyond(h, lens_dev)
    for layer, rnn_layer, rev in plan:
        if rnn_layer is not None:
            if not (hip_rnn_varlen_workspace_bytes(rnn_layer.rnn, h) or hip_lstm_large_workspace_bytes(rnn_layer.rnn, h)):
                return None
            h = rnn_layer(h, reverse=rev, lengths=lens_dev)
            continue
        h = layer(h)
        if isinstance(layer, Convolution):
            lens = conv_out_lengths(lens, layer.stride)
            lens_dev = torch.from_numpy(lens).to(x.device)
        h = _zero_beyond(h, lens_dev)
    return h


def forward_varlen(model, x, lengths):
    """`model` (a `Serial` of this module's layers) on x (T, N, C) whose column n has lengths[n] rows (zero beyond):
    -> (out, out_lengths), where out[:out_lengths[n], n] is what `model(x[:lengths[n], n:n + 1])` gives and every row
    beyond is 0.  out_lengths is a host int64 array (`conv_out_lengths` through every Convolution).  Under grad mode
    (layers.TRAIN_VARLEN = True; a RuntimeError without it) the result is differentiable: the gradient of every parameter, and of x, is the sum over the columns of the gradients
    of those per-column passes (rows of x beyond a column's length get 0).  The loss takes `out_lengths` as its `lengths`
    keyword (`ctc.flipflop_mean_loss`, `ctc.crf_flipflop_loss`, ...: a time length per column; `train.calculate_loss(...,
    lengths=)` is the two calls together).

    On the GPU the batch goes through every layer once: a Convolution's rows beyond the column's output length are
    zeroed (the next window then sees the zeros its own padding would have supplied), the recurrences take the
    lengths (`Lstm` / `GruMod` `forward(x, reverse, lengths)`), the output layers are pointwise per row.  Where a
    recurrent layer has no HIP launch for the tensors (CPU tensors, a size the kernels do not admit, USE_HIP_LSTM or
    USE_HIP_GRU off) every column is evaluated alone at its own length instead."""
    if not isinstance(model, Serial):
        raise TypeError("forward_varlen: the model must be a layers.Serial, not %s" % type(model).__name__)
    plan = _varlen_layers(model)
    if _needs_grad(x, model) and not TRAIN_VARLEN:
        raise RuntimeError("forward_varlen is inference only unless layers.TRAIN_VARLEN is set: call it under "
                           "torch.no_grad(), or set layers.TRAIN_VARLEN = True")
    T, N, _ = x.shape
    lens = np.asarray(lengths.cpu() if torch.is_tensor(lengths) else lengths, dtype=np.int64).reshape(-1)
    if len(lens) != N or (N and (lens.min() < 0 or lens.max() > T)):
        raise ValueError("forward_varlen: lengths must hold one value in 0..%d for each of the %d columns" % (T, N))
    out_lens, t_out = lens, T
    for layer, _, _ in plan:
        if isinstance(layer, Convolution):
            out_lens, t_out = conv_out_lengths(out_lens, layer.stride), conv_out_lengths(t_out, layer.stride)
    last = plan[-1][1] or plan[-1][0]
    nout = last.rnn.hidden_size if isinstance(last, _Rnn) else last.conv.out_channels if isinstance(last, Convolution) \
        else getattr(last, "nout", last.size)
    with torch.enable_grad() if _needs_grad(x, model) else torch.no_grad():
        out = _varlen_batched(plan, x, lens) if T and N else None
        if out is None:
            out = x.new_zeros(t_out, N, nout)
            for n in range(N):
                if lens[n]:
                    out[:out_lens[n], n:n + 1] = model(x[:lens[n], n:n + 1])
    return out, out_lens
