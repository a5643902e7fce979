"""The LSTM forward that saves nothing at hidden size 96 on the matrix cores (include/taiyaki_amd_lstm_matrix.h,
csrc/lstm_matrix.hip, the "matrix" row of layers._rnn_route): 16 columns per workgroup.  Against nn.LSTM in float64 by the
rule of tests/test_lstm_hip.py, bit for bit across batch widths, places in a workgroup and per-column lengths, and the
route by width, grad mode and switch."""
import copy

import pytest
import torch

from taiyaki_amd import _lib, layers

H = 96


def _run(gx, whh, lens, reverse):
    """tk_lstm_matrix_forward_dev -> y, which starts as NaN: a row the kernel does not write shows."""
    T, N, _ = gx.shape
    gx = gx.contiguous()
    y = torch.full((T, N, H), float("nan"), device=gx.device)
    with torch.cuda.device(gx.device):
        rc = _lib.lstm_matrix_lib().tk_lstm_matrix_forward_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(lens), T, N, H,
                                                               int(reverse), _lib.ptr(y), _lib.stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(1, 1), (3, 16), (5, 17), (37, 33), (800, 16)])
@pytest.mark.parametrize("reverse", [False, True])
def test_entry_and_layer_match_float64(gpu_device, monkeypatch, T, N, reverse):
    """(3, 16): one full workgroup; (5, 17): a workgroup with one live column; (800, 16): the longest chunk, where the
    split's error would accumulate.  The error over the largest entry is at most 2 x nn.LSTM's on the device + 2e-6."""
    dev = gpu_device
    monkeypatch.setattr(layers, "LSTM_MATRIX_MIN_COLUMNS", 1)
    torch.manual_seed(T + N)
    lstm = layers.Lstm(20, H)
    x = torch.randn(T, N, 20)
    l64 = copy.deepcopy(lstm).double()
    with torch.no_grad():
        ref = l64(x.double(), reverse=reverse)
        gx64 = x.double() @ l64.rnn.weight_ih_l0.t() + l64.rnn.bias_ih_l0 + l64.rnn.bias_hh_l0
        lstm, xd = lstm.to(dev), x.to(dev)
        before = layers.lstm_matrix_calls["inference"], dict(layers.lstm_local_calls)
        y = lstm(xd, reverse=reverse)
        monkeypatch.setattr(layers, "USE_HIP_LSTM_MATRIX", False)
        monkeypatch.setattr(layers, "USE_HIP_LSTM_LOCAL", False)
        miopen = lstm(xd, reverse=reverse)
        assert (layers.lstm_matrix_calls["inference"], layers.lstm_local_calls) == (before[0] + 1, before[1])
    entry = _run(gx64.float().to(dev), lstm.rnn.weight_hh_l0.detach(), None, reverse)
    scale = ref.abs().max().item()
    e_mio = (miopen.double().cpu() - ref).abs().max().item() / scale
    for what, got in (("layer", y), ("entry", entry)):
        err = (got.double().cpu() - ref).abs().max().item() / scale
        print("T %d N %d rev %d %s: matrix %.3e, nn.LSTM %.3e" % (T, N, reverse, what, err, e_mio))
        assert err <= 2 * e_mio + 2e-6, (what, err, e_mio)


def _case(T, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(T, N, 4 * H, generator=g).to(dev), (torch.randn(4 * H, H, generator=g) / H ** 0.5).to(dev)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_a_column_is_the_same_bits_alone_and_at_another_place(gpu_device, reverse):
    T, N = 23, 37
    gx, whh = _case(T, N, gpu_device, 11)
    batch = _run(gx, whh, None, reverse)
    assert torch.isfinite(batch).all() and batch.abs().max() > 0.1
    for n in range(N):
        assert torch.equal(_run(gx[:, n:n + 1], whh, None, reverse), batch[:, n:n + 1]), n
    moved = torch.roll(gx, 5, dims=1)       # column n at place (n + 5) % 37: another place in another workgroup
    assert torch.equal(torch.roll(_run(moved, whh, None, reverse), -5, dims=1), batch)


VT, VLENS = 41, [41, 0, 1, 20, 40, 41] + [7] * 11 + [0, 33]      # 19 columns: a second workgroup, three of 16 live


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_lengths(gpu_device, reverse):
    dev = gpu_device
    N = len(VLENS)
    gx, whh = _case(VT, N, dev, 12)
    lens = torch.tensor(VLENS, dtype=torch.int32, device=dev)
    beyond = torch.arange(VT, device=dev)[:, None] >= lens[None, :]
    dirty = gx.clone()
    dirty[beyond] = float("nan")
    got = _run(dirty, whh, lens, reverse)
    assert torch.isfinite(got).all(), "a NaN beyond a length reached the output"
    assert not got[beyond].any(), "rows at and beyond the length are 0"
    assert torch.equal(got, _run(gx, whh, lens, reverse))
    for n, ln in enumerate(VLENS):
        if ln:
            assert torch.equal(_run(gx[:ln, n:n + 1], whh, None, reverse), got[:ln, n:n + 1]), n
    full = torch.full((N,), VT, dtype=torch.int32, device=dev)
    assert torch.equal(_run(gx, whh, None, reverse), _run(gx, whh, full, reverse))


@pytest.mark.gpu
@pytest.mark.parametrize("how,matrix", [("at", True), ("below", False), ("grad", False), ("off", False)])
def test_route(gpu_device, monkeypatch, how, matrix):
    """At the threshold under no_grad the layer, with and without lengths, and forward_varlen take the matrix row; one
    column fewer, grad mode and the switch off each take the local one (forward_varlen: every column alone, as before)."""
    dev = gpu_device
    monkeypatch.setattr(layers, "LSTM_MATRIX_MIN_COLUMNS", 20)
    monkeypatch.setattr(layers, "USE_HIP_LSTM_MATRIX", how != "off")
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)
    torch.manual_seed(1)
    lstm = layers.Lstm(12, H).to(dev)
    N = 19 if how == "below" else 20
    x = torch.randn(6, N, 12, device=dev)
    before = layers.lstm_matrix_calls["inference"], sum(layers.lstm_local_calls.values())
    with torch.enable_grad() if how == "grad" else torch.no_grad():
        y = lstm(x)
        yl = lstm(x, lengths=[6] * N)
        yv = layers.forward_varlen(layers.Serial([lstm]), x, [6] * N)[0]
    assert torch.isfinite(y).all() and torch.equal(y, yl) and (y - yv).abs().max().item() < 1e-5
    moved = layers.lstm_matrix_calls["inference"] - before[0], sum(layers.lstm_local_calls.values()) - before[1]
    assert moved == ((3, 0) if matrix else (0, 2 + N)), (how, moved)
