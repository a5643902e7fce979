"""`layers.forward_varlen`: a network pass on columns of different lengths.  On the CPU the pass evaluates every column
alone (its fallback, the oracle of the GPU tests): host logic, the plan of `prepare_mapping_funcs.remap_batch` and the
binding of include/taiyaki_amd_rnn_varlen.h.  On the GPU: the batched pass against every column run alone, under the
project's rule against float64."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, layers, models, prepare_mapping_funcs
from tests.helpers import gru_net

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 2, 4, 5])
@pytest.mark.parametrize("winlen", [5, 19])
def test_conv_out_lengths_is_the_row_count_of_the_layer(winlen, stride):
    torch.manual_seed(0)
    conv = layers.Convolution(1, 3, winlen, stride=stride)
    with torch.no_grad():
        for length in range(1, 61):
            assert conv(torch.randn(length, 1, 1)).shape[0] == layers.conv_out_lengths(length, stride), length
    # 0 stays 0 (the layer itself has no window to place on an empty column), and arrays go through elementwise
    assert layers.conv_out_lengths(0, stride) == 0
    every = np.arange(61)
    assert np.array_equal(layers.conv_out_lengths(every, stride), [layers.conv_out_lengths(int(n), stride) for n in every])
    assert torch.equal(layers.conv_out_lengths(torch.arange(61), stride), torch.from_numpy(-(-every // stride)))


def _padded(T, lengths, seed):
    x = torch.randn(T, len(lengths), 1, generator=torch.Generator().manual_seed(seed))
    for n, ln in enumerate(lengths):
        x[ln:, n] = 0
    return x


@pytest.mark.parametrize("make,stride", [(models.mGru_flipflop, 2), (models.mLstm_flipflop, 5)])
def test_cpu_pass_equals_every_column_run_alone(make, stride):
    torch.manual_seed(1)
    net = make(size=32, stride=stride).eval()
    T, lengths = 64, [64, 0, 1, 3, 33, 63]         # 33 and 63: no multiple of either stride; 3: shorter than any window
    x = _padded(T, lengths, 2)
    with torch.no_grad():
        out, out_len = layers.forward_varlen(net, x, lengths)
        assert out.shape == (-(-T // stride), len(lengths), 40)
        assert np.array_equal(out_len, [-(-n // stride) for n in lengths])
        for n, ln in enumerate(lengths):
            if ln:
                assert torch.equal(out[:out_len[n], n:n + 1], net(x[:ln, n:n + 1])), n
            assert torch.equal(out[out_len[n]:, n], torch.zeros_like(out[out_len[n]:, n])), n
        # a recurrent layer on its own takes lengths too
        h = torch.randn(9, 3, 32)
        for layer in (net[-2], net[-3]):
            y = layer(h, lengths=[9, 0, 4])
            assert torch.equal(y[:4, 2:3], layer(h[:4, 2:3])) and torch.equal(y[:, 0:1], layer(h[:, 0:1]))
            assert not y[:, 1].any() and not y[4:, 2].any()


def test_unknown_layer_type_raises():
    net = layers.Serial([layers.Convolution(1, 8, 5), torch.nn.Tanh()])
    with torch.no_grad(), pytest.raises(TypeError, match="Tanh"):
        layers.forward_varlen(net, torch.zeros(10, 2, 1), [10, 4])
    with torch.no_grad(), pytest.raises(TypeError, match="Convolution"):
        layers.forward_varlen(layers.Serial([layers.Reverse(layers.Convolution(1, 8, 5))]), torch.zeros(10, 2, 1), [10, 4])


def test_lengths_with_gradients_required_raise():
    net = models.mGru_flipflop(size=32, stride=2)
    x = torch.zeros(10, 2, 1)
    with pytest.raises(RuntimeError, match="inference only"):
        layers.forward_varlen(net, x, [10, 4])
    for layer in (layers.GruMod(8, 32), layers.Lstm(8, 32)):
        with pytest.raises(RuntimeError, match="inference only"):
            layer(torch.zeros(10, 2, 8), lengths=[10, 4])
        with pytest.raises(RuntimeError, match="inference only"):
            layers.Reverse(layer)(torch.zeros(10, 2, 8), lengths=[10, 4])
        with torch.no_grad():
            assert layer(torch.zeros(10, 2, 8), lengths=[10, 4]).shape == (10, 2, 32)


@pytest.mark.parametrize("max_columns", [1, 3, 64])
def test_remap_plan(max_columns):
    lengths = np.random.RandomState(3).randint(0, 5000, size=17)
    lengths[5] = lengths[11]                        # a tie
    plan = prepare_mapping_funcs.remap_plan(lengths, max_columns)
    reads = [r for launch in plan for r in launch.reads]
    assert sorted(reads) == list(range(17))
    assert all(1 <= len(launch.reads) <= max_columns for launch in plan)
    assert len(plan) == -(-17 // max_columns)
    assert list(lengths[reads]) == sorted(lengths)
    assert all(launch.nblk == lengths[list(launch.reads)].max() for launch in plan)
    assert prepare_mapping_funcs.remap_plan([], max_columns) == []
    assert prepare_mapping_funcs.remap_plan([123], max_columns) == [prepare_mapping_funcs.Launch((0,), 123)]


def test_varlen_library_exports_exactly_what_its_header_declares():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.VARLEN_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^(?:const\s+)?[a-z_0-9]+\s+\*?\s*([a-z_0-9]+)\(", hdr, flags=re.M))
    assert declared == {"tk_rnn_varlen_workspace_bytes", "tk_lstm_forward_varlen_dev", "tk_gru_forward_varlen_dev"}
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, _lib.VARLEN_LIBNAME)],
                         capture_output=True, text=True, check=True).stdout
    assert {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW"} == declared
    assert set(_lib.VARLEN_SIGNATURES) == declared


def test_varlen_binding_has_the_headers_argument_types():
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert _lib.VARLEN_SIGNATURES == {
        "tk_rnn_varlen_workspace_bytes": (sz, [i, sz, sz, i]),
        "tk_lstm_forward_varlen_dev": (i, [vp, vp, vp, sz, sz, sz, i, i, vp, vp, sz, vp, vp]),
        "tk_gru_forward_varlen_dev": (i, [vp, vp, vp, vp, sz, sz, sz, i, i, vp, vp, sz, vp, vp]),
    }
    assert _lib.VARLEN_DEFINES == {"TK_RNN_KIND_LSTM": 0, "TK_RNN_KIND_GRU": 1}
    V = _lib.varlen_lib()
    assert V.tk_rnn_varlen_workspace_bytes(0, 5, 256, 256) > 0 and V.tk_rnn_varlen_workspace_bytes(1, 5, 96, 256) > 0
    # the admission rules of the existing forwards; an unknown kind runs nowhere
    L = _lib.lib()
    for n, h, cus in [(5, 256, 256), (300, 256, 256), (6, 96, 256), (300, 96, 256), (65, 256, 256), (4, 48, 256), (4, 64, 0)]:
        assert bool(V.tk_rnn_varlen_workspace_bytes(0, n, h, cus)) == bool(L.tk_lstm_workspace_bytes(n, h, cus)), (n, h)
        assert bool(V.tk_rnn_varlen_workspace_bytes(1, n, h, cus)) == bool(L.tk_gru_workspace_bytes(n, h, cus)), (n, h)
        assert V.tk_rnn_varlen_workspace_bytes(2, n, h, cus) == 0


# ---------------------------------------------------------------------------
# GPU: the batched pass against every column alone, both against float64
# ---------------------------------------------------------------------------
def _check_network(net, net64, x, lengths, dev, hip_calls):
    """|out - ref| <= 2 |alone - ref| + 2e-6 max|ref| in max-norm per column (tests/test_gru_hip.py's rule), rows beyond
    out_lengths exactly 0."""
    with torch.no_grad():
        xg = x.to(dev)
        out, out_len = layers.forward_varlen(net, xg, lengths)
        assert hip_calls() > 0, "the batched pass took no HIP launch"
        assert np.array_equal(out_len, prepare_mapping_funcs.network_out_lengths(net, lengths))
        assert out.shape[:2] == (out_len.max(), len(lengths)) and torch.isfinite(out).all()
        for n, ln in enumerate(lengths):
            assert torch.equal(out[out_len[n]:, n], torch.zeros_like(out[out_len[n]:, n])), n
            if ln == 0:
                continue
            alone = net(xg[:ln, n:n + 1]).double().cpu()
            ref = net64(x[:ln, n:n + 1].double())
            got = out[:out_len[n], n:n + 1].double().cpu()
            assert got.shape == ref.shape == alone.shape
            scale = ref.abs().max().item()
            e_out, e_alone = (got - ref).abs().max().item(), (alone - ref).abs().max().item()
            print("column %d (%d samples): |out - ref| %.3g, |alone - ref| %.3g, max|ref| %.3g" % (n, ln, e_out, e_alone, scale))
            assert e_out <= 2 * e_alone + 2e-6 * scale, (n, e_out, e_alone, scale)


class _count_varlen_launches:
    """Counts the calls of layers._rnn_forward_varlen that reach a HIP launch (a non-zero workspace)."""

    def __init__(self, monkeypatch):
        self.n = 0
        real = layers.hip_rnn_varlen_workspace_bytes

        def counted(rnn, x):
            wsb = real(rnn, x)
            self.n += bool(wsb)
            return wsb
        monkeypatch.setattr(layers, "hip_rnn_varlen_workspace_bytes", counted)

    def __call__(self):
        return self.n


@pytest.mark.gpu
def test_shipped_gru_network_columns_match_float64(gpu_device, monkeypatch):
    arrays = gru_net.load_arrays()
    lengths = [2000, 1999, 1001, 19, 3, 0]
    x = torch.from_numpy(arrays["signal"][:, :6].copy()).unsqueeze(2)
    for n, ln in enumerate(lengths):
        x[ln:, n] = 0
    net, net64 = gru_net.build_model(arrays).to(gpu_device), gru_net.build_model(arrays, torch.float64)
    _check_network(net, net64, x, lengths, gpu_device, _count_varlen_launches(monkeypatch))


@pytest.mark.gpu
def test_lstm_network_on_the_narrow_convolutions_matches_float64(gpu_device, monkeypatch):
    import copy
    torch.manual_seed(11)
    net = models.mLstm_flipflop(size=64, stride=5).eval()
    net64 = copy.deepcopy(net).double()
    lengths = [600, 598, 301, 7, 0]
    x = _padded(600, lengths, 12)
    net = net.to(gpu_device)
    assert net[0]._hip_small(x.to(gpu_device)), "the narrow HIP convolution does not take the input"
    _check_network(net, net64, x, lengths, gpu_device, _count_varlen_launches(monkeypatch))
