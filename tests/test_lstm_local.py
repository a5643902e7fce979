"""The LSTM recurrence at hidden size 96 (include/taiyaki_amd_lstm_local.h, csrc/lstm_local.hip, layers.LstmRecurrence on
the "local" rows of layers._RNN_LAUNCHES): one workgroup owns every unit of its columns.  Against nn.LSTM in float64 by the rule of tests/test_lstm_hip.py, and bit
for bit across batch widths, columns per workgroup and per-column lengths."""
import copy
import ctypes

import pytest
import torch

from taiyaki_amd import _lib, layers

H = 96


def _columns(N, dev):
    """The columns per workgroup the release rule picks for a batch of N on this device, from the library's own query."""
    cus = layers._cu_count(dev)
    C = _lib.lstm_local_lib().tk_lstm_local_columns(N, H, cus)
    assert C == (1 if N <= cus else 2), (N, cus, C)
    return C


class _nn_lstm:
    """USE_HIP_LSTM_LOCAL = False inside: nn.LSTM on the same device."""

    def __enter__(self):
        self.old, layers.USE_HIP_LSTM_LOCAL = layers.USE_HIP_LSTM_LOCAL, False

    def __exit__(self, *exc):
        layers.USE_HIP_LSTM_LOCAL = self.old


def _named(module):
    return [(k, p) for k, p in module.named_parameters() if p.requires_grad]


def _grads(module, call, x, dy):
    """y = call(x) and d (y * dy).sum() / d (x, every parameter of `module` that requires a gradient)."""
    x = x.detach().clone().requires_grad_(True)
    for _, p in _named(module):
        p.grad = None
    y = call(x)
    (y * dy).sum().backward()
    out = {"y": y, "x": x.grad}
    out.update({k: p.grad for k, p in _named(module)})
    return {k: v.detach().clone() for k, v in out.items()}


def _assert_rule(ref, hip, miopen, what):
    """tests/test_lstm_hip.py::_compare: the largest error against float64 over the tensor's largest entry is at most
    2 x nn.LSTM's on the same device + 2e-6."""
    assert set(ref) == set(hip) == set(miopen)
    for k, r in ref.items():
        scale = r.abs().max().item() or 1.0         # (dW_hh is 0 at T = 1)
        e_hip = (hip[k].double().cpu() - r).abs().max().item() / scale
        e_mio = (miopen[k].double().cpu() - r).abs().max().item() / scale
        print("%s %s: local %.3e, nn.LSTM %.3e, ratio %.3f" % (what, k, e_hip, e_mio, e_hip / (2 * e_mio + 2e-6)))
        assert e_hip <= 2 * e_mio + 2e-6, (what, k, e_hip, e_mio)


# ---------------------------------------------------------------------------------------------------------------------
# against float64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("T,N,I", [(1, 1, 7), (2, 3, 96), (37, 5, 20), (25, 70, 96), (5, 300, 16), (800, 4, 96)])
@pytest.mark.parametrize("reverse", [False, True])
def test_layer_matches_float64(gpu_device, T, N, I, reverse):
    """y, dx, dW_ih, dW_hh and db_ih of one layer.  (5, 300, 16): N above the CU count, two columns per workgroup, the
    last workgroup's second column empty; (800, 4, 96): the fast model's longest chunk."""
    dev = gpu_device
    torch.manual_seed(0)
    lstm = layers.Lstm(I, H)
    layer = layers.Reverse(lstm) if reverse else lstm
    x = torch.randn(T, N, I)
    dy = torch.randn(T, N, H) / (T * N) ** 0.5
    l64 = copy.deepcopy(layer).double()
    ref = _grads(l64, l64, x.double(), dy.double())
    layer = layer.to(dev)
    C = _columns(N, dev)
    assert layers.hip_lstm_workspace_bytes(lstm.rnn, x.to(dev)) == 0 and layers.hip_lstm_local_takes(lstm.rnn, x.to(dev))
    before = dict(layers.lstm_local_calls)
    hip = _grads(layer, layer, x.to(dev), dy.to(dev))
    assert layers.lstm_local_calls["saved"] == before["saved"] + 1, ("C", C)
    with _nn_lstm():
        miopen = _grads(layer, layer, x.to(dev), dy.to(dev))
    assert layers.lstm_local_calls["saved"] == before["saved"] + 1, "the switch"
    _assert_rule(ref, hip, miopen, "T %d N %d I %d rev %d C %d" % (T, N, I, reverse, C))


# ---------------------------------------------------------------------------------------------------------------------
# the C entries: bits
# ---------------------------------------------------------------------------------------------------------------------
def _case(T, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    gx = torch.randn(T, N, 4 * H, generator=g).to(dev)
    whh = (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)
    dy = torch.randn(T, N, H, generator=g).to(dev)
    return gx, whh, dy


def _run(gx, whh, dy, lens, reverse, save=True):
    """The forward (save: and the backward) through the C entries -> dict of y (, gates, cell, dgates).  The outputs start
    as NaN: a row the kernels do not write shows."""
    L = _lib.lstm_local_lib()
    T, N, _ = gx.shape
    dev = gx.device
    cus = layers._cu_count(dev)
    gx, dy = gx.contiguous(), dy.contiguous()
    nan = float("nan")
    out = {"y": torch.full((T, N, H), nan, device=dev)}
    if save:
        out.update(gates=torch.full((T, N, 4 * H), nan, device=dev), cell=torch.full((T, N, H), nan, device=dev),
                   dgates=torch.full((T, N, 4 * H), nan, device=dev))
    p = _lib.ptr
    with torch.cuda.device(dev):
        rc = L.tk_lstm_local_forward_dev(p(gx), p(whh), p(lens), T, N, H, int(reverse), cus, p(out["y"]),
                                         p(out.get("gates")), p(out.get("cell")), _lib.stream_ptr())
        assert rc == 0, rc
        if save:
            rc = L.tk_lstm_local_backward_dev(p(whh), p(out["gates"]), p(out["cell"]), p(dy), p(lens), T, N, H,
                                              int(reverse), cus, p(out["dgates"]), _lib.stream_ptr())
            assert rc == 0, rc
        torch.cuda.synchronize()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_a_column_is_the_same_bits_alone_and_at_either_column_count(gpu_device, labenv, reverse):
    T, N = 23, 7
    gx, whh, dy = _case(T, N, gpu_device, 11)
    batch = _run(gx, whh, dy, None, reverse)
    assert all(torch.isfinite(v).all() for v in batch.values())
    assert batch["y"].abs().max() > 0.1 and batch["dgates"].abs().max() > 1e-3
    for n in range(N):
        alone = _run(gx[:, n:n + 1], whh, dy[:, n:n + 1], None, reverse)
        for k, v in alone.items():
            assert torch.equal(v, batch[k][:, n:n + 1]), (k, n)
    labenv.lib()
    L = _lib.lstm_local_lib()
    try:
        forced = {}
        for C in (1, 2):
            L.tk_lab_lstm_local_cols(C)
            assert L.tk_lstm_local_columns(N, H, layers._cu_count(gpu_device)) == C
            forced[C] = _run(gx, whh, dy, None, reverse)
    finally:
        L.tk_lab_lstm_local_cols(0)
    for k, v in batch.items():
        assert torch.equal(forced[1][k], v) and torch.equal(forced[2][k], v), k


# ---------------------------------------------------------------------------------------------------------------------
# lengths
# ---------------------------------------------------------------------------------------------------------------------
VT, VLENS = 41, [41, 0, 1, 20, 40, 41]


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_lengths_at_the_c_entries(gpu_device, reverse):
    dev = gpu_device
    N = len(VLENS)
    gx, whh, dy = _case(VT, N, dev, 12)
    lens = torch.tensor(VLENS, dtype=torch.int32, device=dev)
    beyond = torch.arange(VT, device=dev)[:, None] >= lens[None, :]
    dirty_gx, dirty_dy = gx.clone(), dy.clone()
    dirty_gx[beyond] = float("nan")
    dirty_dy[beyond] = float("nan")
    got = _run(dirty_gx, whh, dirty_dy, lens, reverse)
    for k, v in got.items():
        assert torch.isfinite(v).all(), (k, "a NaN beyond a length reached the output")
        assert not v[beyond].any(), (k, "rows at and beyond the length are 0")
    for n, ln in enumerate(VLENS):
        if ln:
            alone = _run(gx[:ln, n:n + 1], whh, dy[:ln, n:n + 1], None, reverse)
            for k, v in alone.items():
                assert torch.equal(v, got[k][:ln, n:n + 1]), (k, n)
    # nothing saved: the same y
    assert torch.equal(_run(dirty_gx, whh, dirty_dy, lens, reverse, save=False)["y"], got["y"])
    # no lengths: every column has T steps
    full = torch.full((N,), VT, dtype=torch.int32, device=dev)
    a, b = _run(gx, whh, dy, None, reverse), _run(gx, whh, dy, full, reverse)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(_run(gx, whh, dy, None, reverse, save=False)["y"], a["y"])


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_lengths_through_the_layer(gpu_device, monkeypatch, reverse):
    dev = gpu_device
    torch.manual_seed(13)
    layer = layers.Lstm(20, H)
    N = len(VLENS)
    x, dy = torch.randn(VT, N, 20), torch.randn(VT, N, H)
    for n, ln in enumerate(VLENS):
        x[ln:, n] = 0
    l64 = copy.deepcopy(layer).double()

    def columns(module, x, dy):
        """every column alone at its own length: y column by column, the parameter gradients summed in float64"""
        acc = {"y": torch.zeros(VT, N, H, dtype=torch.float64)}
        for n, ln in enumerate(VLENS):
            if ln:
                g = _grads(module, lambda v: module(v, reverse=reverse), x[:ln, n:n + 1].contiguous(),
                           dy[:ln, n:n + 1].contiguous())
                acc["y"][:ln, n:n + 1] = g.pop("y").double().cpu()
                g.pop("x")
                for k, v in g.items():
                    acc[k] = acc.get(k, 0) + v.double().cpu()
        return acc

    ref = columns(l64, x.double(), dy.double())
    layer = layer.to(dev)
    xd, dyd = x.to(dev), dy.to(dev)
    # inference: the launch that saves nothing
    before = dict(layers.lstm_local_calls)
    with torch.no_grad():
        y = layer(xd, reverse=reverse, lengths=VLENS)
    assert layers.lstm_local_calls == {"saved": before["saved"], "inference": before["inference"] + 1}
    beyond = torch.arange(VT)[:, None] >= torch.tensor(VLENS)[None, :]
    assert not y.cpu()[beyond].any() and (y.double().cpu() - ref["y"]).abs().max().item() < 1e-5
    # under grad mode the call raises without the switch ...
    assert layers.TRAIN_VARLEN is False
    with pytest.raises(RuntimeError, match="TRAIN_VARLEN"):
        layer(xd, reverse=reverse, lengths=VLENS)
    # ... and with it trains: the parameter gradients are the sum of the per-column calls
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)
    hip = _grads(layer, lambda v: layer(v, reverse=reverse, lengths=VLENS), xd, dyd)
    assert layers.lstm_local_calls["saved"] == before["saved"] + 1
    hip.pop("x")
    with _nn_lstm():
        alone = columns(layer, xd, dyd)
    _assert_rule(ref, hip, alone, "lengths rev %d" % reverse)


# ---------------------------------------------------------------------------------------------------------------------
# the model, and a captured forward
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_fast_model_matches_float64(gpu_device):
    """models.mLstm_flipflop(size=96), the reference's fast model: scores and every parameter gradient."""
    from taiyaki_amd import models
    dev = gpu_device
    torch.manual_seed(96)
    net = models.mLstm_flipflop(size=H)
    x, dy = torch.randn(500, 6, 1), torch.randn(100, 6, 40) / 600 ** 0.5
    n64 = copy.deepcopy(net).double()
    ref = _grads(n64, n64, x.double(), dy.double())
    net = net.to(dev)
    before = dict(layers.lstm_local_calls)
    hip = _grads(net, net, x.to(dev), dy.to(dev))
    assert layers.lstm_local_calls == {"saved": before["saved"] + 5, "inference": before["inference"]}
    with _nn_lstm():
        miopen = _grads(net, net, x.to(dev), dy.to(dev))
    for d in (ref, hip, miopen):
        d.pop("x")                                  # (the network's input requires no gradient in training)
    assert len(ref) == 1 + 6 + 15 + 2
    _assert_rule(ref, hip, miopen, "mLstm_flipflop 96")
    with torch.no_grad():
        y = net(x.to(dev))
    assert layers.lstm_local_calls == {"saved": before["saved"] + 5, "inference": before["inference"] + 5}
    assert (y - hip["y"]).abs().max().item() <= 1e-5 * hip["y"].abs().max().item()


@pytest.mark.gpu
def test_captured_forward_replays_bit_identical(gpu_device):
    """tests/test_lstm_hip.py's captured forward at size 96: a single stream, three replays."""
    torch.manual_seed(7)
    layer = layers.Serial([layers.Reverse(layers.Lstm(32, H)), layers.Lstm(H, H)]).to(gpu_device)
    x = torch.randn(90, 21, 32, device=gpu_device)
    before = layers.lstm_local_calls["inference"]
    with torch.no_grad():
        eager = layer(x)
        assert layers.lstm_local_calls["inference"] == before + 2
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            layer(x)
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = layer(x)
        for _ in range(3):
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
