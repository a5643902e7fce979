"""The GRU forward that saves nothing at hidden size 96 on the matrix cores (include/taiyaki_amd_gru_matrix.h,
csrc/gru_matrix.hip, the "gru_matrix" row of layers._rnn_route): 16 columns per workgroup.  Against nn.GRU in float64 by
the rule of tests/test_gru_hip.py, bit for bit across batch widths, places in a workgroup and per-column lengths, the
route by width, grad mode and switch, and the reference's shipped network."""
import copy

import pytest
import torch

from taiyaki_amd import _lib, decode, layers
from tests.helpers import gru_net

H = 96


def _run(gx, whh, bhh, lens, reverse):
    """tk_gru_matrix_forward_dev -> y, which starts as NaN: a row the kernel does not write shows."""
    T, N, _ = gx.shape
    gx = gx.contiguous()
    y = torch.full((T, N, H), float("nan"), device=gx.device)
    with torch.cuda.device(gx.device):
        rc = _lib.gru_matrix_lib().tk_gru_matrix_forward_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(bhh), _lib.ptr(lens), T,
                                                             N, H, int(reverse), _lib.ptr(y), _lib.stream_ptr())
        assert rc == 0, rc
        torch.cuda.synchronize()
    return y


@pytest.mark.gpu
@pytest.mark.parametrize("T,N", [(1, 1), (3, 16), (5, 17), (37, 33), (800, 16)])
@pytest.mark.parametrize("reverse", [False, True])
def test_entry_and_layer_match_float64(gpu_device, monkeypatch, T, N, reverse):
    """(3, 16): one full workgroup; (5, 17): one live column; (800, 16): the longest chunk.  b_hh is live, so bhh_n's
    place inside the reset product counts.  Error over the largest entry <= 2 x nn.GRU's on the device + 2e-6."""
    dev = gpu_device
    monkeypatch.setattr(layers, "GRU_MATRIX_MIN_COLUMNS", 1)
    monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX", True)
    torch.manual_seed(T + N)
    gru = layers.GruMod(20, H)
    with torch.no_grad():
        gru.rnn.bias_hh_l0.normal_(0.0, 0.5)
    x = torch.randn(T, N, 20)
    g64 = copy.deepcopy(gru).double()
    with torch.no_grad():
        ref = g64(x.double(), reverse=reverse)
        gx64 = x.double() @ g64.rnn.weight_ih_l0.t() + g64.rnn.bias_ih_l0
        gru, xd = gru.to(dev), x.to(dev)
        before = layers.gru_matrix_calls["inference"]
        y = gru(xd, reverse=reverse)
        assert layers.gru_matrix_calls["inference"] == before + 1
        monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX", False)
        monkeypatch.setattr(layers, "USE_HIP_GRU", False)
        miopen = gru(xd, reverse=reverse)
        assert layers.gru_matrix_calls["inference"] == before + 1
    entry = _run(gx64.float().to(dev), gru.rnn.weight_hh_l0.detach(), gru.rnn.bias_hh_l0.detach(), None, reverse)
    scale = ref.abs().max().item()
    e_mio = (miopen.double().cpu() - ref).abs().max().item() / scale
    for what, got in (("layer", y), ("entry", entry)):
        err = (got.double().cpu() - ref).abs().max().item() / scale
        print("T %d N %d rev %d %s: matrix %.3e, nn.GRU %.3e" % (T, N, reverse, what, err, e_mio))
        assert err <= 2 * e_mio + 2e-6, (what, err, e_mio)


def _case(T, N, dev, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(T, N, 3 * H, generator=g).to(dev), (torch.randn(3 * H, H, generator=g) / H ** 0.5).to(dev),
            (0.5 * torch.randn(3 * H, generator=g)).to(dev))


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_a_column_is_the_same_bits_alone_and_at_another_place(gpu_device, reverse):
    T, N = 23, 37
    gx, whh, bhh = _case(T, N, gpu_device, 11)
    batch = _run(gx, whh, bhh, None, reverse)
    assert torch.isfinite(batch).all() and batch.abs().max() > 0.1
    for n in range(N):
        assert torch.equal(_run(gx[:, n:n + 1], whh, bhh, None, reverse), batch[:, n:n + 1]), n
    moved = torch.roll(gx, 5, dims=1)       # column n at place (n + 5) % 37: another place in another workgroup
    assert torch.equal(torch.roll(_run(moved, whh, bhh, None, reverse), -5, dims=1), batch)


VT, VLENS = 41, [41, 0, 1, 20, 40, 41] + [7] * 11 + [0, 33]      # 19 columns: a second workgroup, three of 16 live


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_lengths(gpu_device, reverse):
    dev = gpu_device
    N = len(VLENS)
    gx, whh, bhh = _case(VT, N, dev, 12)
    lens = torch.tensor(VLENS, dtype=torch.int32, device=dev)
    beyond = torch.arange(VT, device=dev)[:, None] >= lens[None, :]
    dirty = gx.clone()
    dirty[beyond] = float("nan")
    got = _run(dirty, whh, bhh, lens, reverse)
    assert torch.isfinite(got).all(), "a NaN beyond a length reached the output"
    assert not got[beyond].any(), "rows at and beyond the length are 0"
    assert torch.equal(got, _run(gx, whh, bhh, lens, reverse))
    for n, ln in enumerate(VLENS):
        if ln:
            assert torch.equal(_run(gx[:ln, n:n + 1], whh, bhh, None, reverse), got[:ln, n:n + 1]), n
    full = torch.full((N,), VT, dtype=torch.int32, device=dev)
    assert torch.equal(_run(gx, whh, bhh, None, reverse), _run(gx, whh, bhh, full, reverse))


@pytest.mark.gpu
@pytest.mark.parametrize("how,matrix", [("at", True), ("below", False), ("grad", False), ("off", False)])
def test_route(gpu_device, monkeypatch, how, matrix):
    """At the threshold under no_grad the layer, with and without lengths, and forward_varlen take the row."""
    dev = gpu_device
    monkeypatch.setattr(layers, "GRU_MATRIX_MIN_COLUMNS", 20)
    monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX", how != "off")
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)
    torch.manual_seed(1)
    gru = layers.GruMod(12, H).to(dev)
    N = 19 if how == "below" else 20
    x = torch.randn(6, N, 12, device=dev)
    before = layers.gru_matrix_calls["inference"]
    with torch.enable_grad() if how == "grad" else torch.no_grad():
        y = gru(x)
        yl = gru(x, lengths=[6] * N)
        yv = layers.forward_varlen(layers.Serial([gru]), x, [6] * N)[0]
    assert torch.isfinite(y).all() and (y - yl).abs().max().item() < 1e-5 and (y - yv).abs().max().item() < 1e-5
    assert layers.gru_matrix_calls["inference"] - before == (3 if matrix else 0) and (torch.equal(y, yl) or not matrix)


@pytest.mark.gpu
def test_the_shipped_network(gpu_device, monkeypatch):
    """The reference's five GRU layers of size 96 on their 16 chunks: by the rule above against the existing kernels."""
    monkeypatch.setattr(layers, "GRU_MATRIX_MIN_COLUMNS", 16)
    arrays = gru_net.load_arrays()
    signal = torch.from_numpy(arrays["signal"]).unsqueeze(2)
    with torch.no_grad():
        ref = gru_net.build_model(arrays, torch.float64)(signal.double())
        net, xg = gru_net.build_model(arrays).to(gpu_device), signal.to(gpu_device)
        before = layers.gru_matrix_calls["inference"]
        monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX", True)
        on = net(xg)
        assert layers.gru_matrix_calls["inference"] == before + 5
        monkeypatch.setattr(layers, "USE_HIP_GRU_MATRIX", False)
        off = net(xg)
        assert layers.gru_matrix_calls["inference"] == before + 5
    scale = ref.abs().max().item()
    e_on, e_off = ((s.double().cpu() - ref).abs().max().item() / scale for s in (on, off))
    paths = [decode.flipflop_viterbi(s.contiguous())[2] for s in (on, off)]
    differ = paths[0] != paths[1]
    gap = (on - off).abs().max().item()
    print("shipped network: matrix %.3e, existing %.3e; %d of %d path positions differ; largest score gap %.3e"
          % (e_on, e_off, int(differ.sum()), differ.numel(), gap))
    assert e_on <= 2 * e_off + 2e-6, (e_on, e_off)
    assert not differ.any(), (int(differ.sum()), differ.numel(), gap)
