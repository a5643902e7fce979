"""layers.Lstm's recurrence on the HIP kernels (csrc/lstm_kernels.hip, layers.LstmRecurrence) against nn.LSTM."""
import pytest
import torch

from taiyaki_amd import _lib, layers


def test_geometry_covers_the_model_sizes_and_refuses_the_rest():
    """tk_lstm_workspace_bytes: 0 where the kernels do not run.  Sizes 16 .. 256 (powers of two), any batch whose
    groups of 8 or 16 columns fit one workgroup per CU."""
    L = _lib.lib()
    ws = L.tk_lstm_workspace_bytes
    # 16 groups of 8 columns x 16 workgroups; the backward's reduce-scatter buffer: 2 slots x 16 x 16 x 8 x 256 x 8 B
    assert ws(128, 256, 256) == 2 * 16 * 16 * 8 * 256 * 8
    assert ws(171, 256, 256) == 2 * 11 * 16 * 16 * 256 * 8         # > 256 workgroups at 8 columns: 16 columns
    for n, h in [(1, 16), (5, 16), (6, 32), (70, 32), (64, 256), (8, 64), (128, 128)]:
        assert ws(n, h, 256) > 0, (n, h)
    for n, h in [(300, 256), (128, 8), (128, 96), (128, 512), (0, 256)]:
        assert ws(n, h, 256) == 0, (n, h)
    assert ws(128, 256, 128) == 2 * 8 * 16 * 16 * 256 * 8
    assert ws(128, 256, 0) == 0


def test_cpu_tensors_and_the_switch_take_nn_lstm():
    torch.manual_seed(0)
    layer = layers.Reverse(layers.Lstm(12, 16))
    x = torch.randn(9, 3, 12)
    assert layers.hip_lstm_workspace_bytes(layer.layer.rnn, x) == 0
    ref = torch.flip(layer.layer.rnn(torch.flip(x, (0,)))[0], (0,))
    assert torch.equal(layer(x), ref)
    assert list(layer.state_dict()) == ["layer.rnn.weight_ih_l0", "layer.rnn.weight_hh_l0", "layer.rnn.bias_ih_l0",
                                        "layer.rnn.bias_hh_l0"]
    old = layers.USE_HIP_LSTM
    try:
        layers.USE_HIP_LSTM = False
        assert layers.hip_lstm_workspace_bytes(layer.layer.rnn, x) == 0
    finally:
        layers.USE_HIP_LSTM = old


def _grads(layer, x, dy):
    x = x.detach().clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    y = layer(x)
    (y * dy).sum().backward()
    rnn = layer.layer.rnn if isinstance(layer, layers.Reverse) else layer.rnn
    out = {"y": y, "x": x.grad, "w_ih": rnn.weight_ih_l0.grad, "w_hh": rnn.weight_hh_l0.grad, "b_ih": rnn.bias_ih_l0.grad}
    return {k: v.detach().clone() for k, v in out.items()}      # (the module's .to() would move the .grad tensors)


def _compare(T, N, H, I, reverse, dev, seed=0):
    torch.manual_seed(seed)
    lstm = layers.Lstm(I, H)
    layer = layers.Reverse(lstm) if reverse else lstm
    x = torch.randn(T, N, I)
    dy = torch.randn(T, N, H) / (T * N) ** 0.5
    ref = _grads(layer.double(), x.double(), dy.double())
    layer = layer.float().to(dev)
    assert layers.hip_lstm_workspace_bytes(lstm.rnn, x.to(dev)) > 0
    hip = _grads(layer, x.to(dev), dy.to(dev))
    old = layers.USE_HIP_LSTM
    try:
        layers.USE_HIP_LSTM = False
        miopen = _grads(layer, x.to(dev), dy.to(dev))
    finally:
        layers.USE_HIP_LSTM = old
    for k, r in ref.items():
        scale = r.abs().max().item() or 1.0         # (dW_hh is 0 at T = 1)
        e_hip = (hip[k].double().cpu() - r).abs().max().item() / scale
        e_mio = (miopen[k].double().cpu() - r).abs().max().item() / scale
        assert e_hip <= 2 * e_mio + 2e-6, (T, N, H, reverse, k, e_hip, e_mio)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", [(1, 5, 16, 7), (37, 5, 16, 16), (50, 6, 32, 32), (25, 70, 32, 20),
                                     (40, 8, 64, 64), (30, 37, 128, 16), (20, 130, 256, 256)])
@pytest.mark.parametrize("reverse", [False, True])
def test_small_and_ragged_shapes_match_float64(gpu_device, T, N, H, I, reverse):
    _compare(T, N, H, I, reverse, gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_config2_layer_matches_float64(gpu_device, reverse):
    """The flagship's layer: T = 800, N = 128, H = 256 at the layer's own initialisation."""
    _compare(800, 128, 256, 256, reverse, gpu_device, seed=3)


@pytest.mark.gpu
def test_lab_geometry_16_columns_matches_8(gpu_device):
    """The two launch geometries (8 or 16 batch columns per workgroup) agree to rounding (the backward's
    reduce-scatter sums its producers in two interleaved halves at 8 columns, in one run at 16)."""
    torch.manual_seed(5)
    layer = layers.Reverse(layers.Lstm(64, 256)).to(gpu_device)
    x = torch.randn(60, 40, 64, device=gpu_device)
    dy = torch.randn(60, 40, 256, device=gpu_device)
    L = _lib.use_lab(True)
    try:
        L.tk_lab_lstm_cols(8)
        a = _grads(layer, x, dy)
        L.tk_lab_lstm_cols(16)
        b = _grads(layer, x, dy)
    finally:
        L.tk_lab_lstm_cols(0)
        _lib.use_lab(False)
    for k in a:
        assert (a[k] - b[k]).abs().max().item() <= 1e-5 * a[k].abs().max().item(), k


@pytest.mark.gpu
def test_captured_forward_replays_bit_identical(gpu_device):
    torch.manual_seed(7)
    layer = layers.Serial([layers.Reverse(layers.Lstm(32, 64)), layers.Lstm(64, 64)]).to(gpu_device)
    x = torch.randn(90, 21, 32, device=gpu_device)
    strict = _lib.is_strict()
    _lib.set_strict(False)
    try:
        with torch.no_grad():
            eager = layer(x)
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
        _lib.raise_if_nonfinite()
    finally:
        _lib.set_strict(strict)
