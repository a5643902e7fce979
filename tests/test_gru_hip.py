"""layers.GruMod's recurrence on the HIP kernels (csrc/gru_kernels.hip, layers.GruRecurrence) against nn.GRU, and the
reference's shipped mGru network (tests/golden/gru_net*.npz) through this repository's model."""
import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, layers
from tests.helpers import gru_net


def test_geometry_covers_the_model_sizes_and_refuses_the_rest():
    """tk_gru_workspace_bytes: 0 where the kernels do not run, never 0 where they do.  Sizes 32, 64, 96 and 128 are
    one workgroup per 1 or 2 batch columns (any batch); size 256 is groups of 4 workgroups that wait for each other, so
    ceil(N / 4) * 4 workgroups must fit one per CU."""
    ws = _lib.lib().tk_gru_workspace_bytes
    for n, h in [(64, 96), (128, 256), (1, 32), (37, 128), (5, 64), (4000, 96), (256, 256), (1, 256)]:
        assert ws(n, h, 256) > 0, (n, h)
    for n, h in [(0, 96), (0, 256), (64, 80), (64, 512), (64, 16), (64, 0), (257, 256)]:
        assert ws(n, h, 256) == 0, (n, h)
    assert ws(64, 96, 0) == 0 and ws(128, 256, 0) == 0 and ws(64, 96, -1) == 0
    # the backward's reduce-scatter buffer at size 256: 2 slots x 32 groups x 4 producers x 4 columns x 256 x 8 B
    assert ws(128, 256, 256) == 2 * 32 * 4 * 4 * 256 * 8
    assert ws(128, 256, 127) == 0 and ws(128, 256, 128) > 0
    assert ws(4000, 96, 1) > 0          # nothing is handed between workgroups: no residency condition


def test_cpu_tensors_and_the_switch_take_nn_gru():
    torch.manual_seed(0)
    layer = layers.Reverse(layers.GruMod(12, 32))
    x = torch.randn(9, 3, 12)
    assert layers.USE_HIP_GRU is True
    assert layers.hip_gru_workspace_bytes(layer.layer.rnn, x) == 0
    ref = torch.flip(layer.layer.rnn(torch.flip(x, (0,)))[0], (0,))
    assert torch.equal(layer(x), ref)
    assert torch.equal(layer.layer(x), layer.layer.rnn(x)[0])
    assert list(layer.state_dict()) == ["layer.rnn.weight_ih_l0", "layer.rnn.weight_hh_l0", "layer.rnn.bias_ih_l0",
                                        "layer.rnn.bias_hh_l0"]
    assert list(layers.GruMod(12, 32).state_dict()) == ["rnn.weight_ih_l0", "rnn.weight_hh_l0", "rnn.bias_ih_l0",
                                                        "rnn.bias_hh_l0"]
    old = layers.USE_HIP_GRU
    try:
        layers.USE_HIP_GRU = False
        assert layers.hip_gru_workspace_bytes(layer.layer.rnn, x) == 0
        assert torch.equal(layer(x), ref)
    finally:
        layers.USE_HIP_GRU = old


def test_trained_network_from_the_fixture_reproduces_its_scores_on_the_cpu():
    """The repository's model with the checkpoint's parameters, CPU fp32, against the genuine network's fp32 CPU
    scores.  Both sides are torch CPU nn.GRU on the same weights; the difference measured when the fixture was made
    was 0.0 (make_golden_gru_net.py), so the bound is the floor: 4 x 0.0 -> 5e-6 on scores that span +-5."""
    arrays = gru_net.load_arrays()
    assert arrays["signal"].shape == (2000, 16) and arrays["scores"].shape == (500, 16, 40)
    assert sum(v.size for k, v in arrays.items() if k.startswith("param/")) == 285160
    net = gru_net.build_model(arrays)
    with torch.no_grad():
        got = net(torch.from_numpy(arrays["signal"]).unsqueeze(2)).numpy()
    diff = np.abs(got - arrays["scores"]).max()
    print("trained network, CPU fp32 against the fixture's scores: max-abs %.3g" % diff)
    assert diff <= 5e-6, diff


def _rnn(layer):
    return layer.layer.rnn if isinstance(layer, layers.Reverse) else layer.rnn


def _grads(layer, x, dy):
    x = x.detach().clone().requires_grad_(True)
    for p in layer.parameters():
        p.grad = None
    y = layer(x)
    (y * dy).sum().backward()
    rnn = _rnn(layer)
    out = {"y": y, "x": x.grad, "w_ih": rnn.weight_ih_l0.grad, "w_hh": rnn.weight_hh_l0.grad,
           "b_ih": rnn.bias_ih_l0.grad}
    if rnn.bias_hh_l0.requires_grad:
        out["b_hh"] = rnn.bias_hh_l0.grad
    return {k: v.detach().clone() for k, v in out.items()}      # (the module's .to() would move the .grad tensors)


def _assert_within_twice_miopen(ref, hip, miopen, what):
    """tests/test_lstm_hip.py::_compare's rule: error relative to the tensor's max-abs, HIP <= 2 x MIOpen + 2e-6."""
    for k, r in ref.items():
        scale = r.abs().max().item() or 1.0         # (dW_hh is 0 at T = 1)
        e_hip = (hip[k].double().cpu() - r).abs().max().item() / scale
        e_mio = (miopen[k].double().cpu() - r).abs().max().item() / scale
        print("%s %s: hip %.3g miopen %.3g" % (what, k, e_hip, e_mio))
        assert e_hip <= 2 * e_mio + 2e-6, (what, k, e_hip, e_mio)


def _compare(T, N, H, I, reverse, dev, seed=0, live_bias_hh=False):
    torch.manual_seed(seed)
    gru = layers.GruMod(I, H)
    if live_bias_hh:                                # any nn.GRU state: bhh_n sits inside r * (...), db_hh has its own sum
        with torch.no_grad():
            gru.rnn.bias_hh_l0.normal_(0.0, 0.5)
        gru.rnn.bias_hh_l0.requires_grad_(True)
    layer = layers.Reverse(gru) if reverse else gru
    x = torch.randn(T, N, I)
    dy = torch.randn(T, N, H) / (T * N) ** 0.5
    ref = _grads(layer.double(), x.double(), dy.double())
    layer = layer.float().to(dev)
    assert layers.hip_gru_workspace_bytes(gru.rnn, x.to(dev)) > 0
    hip = _grads(layer, x.to(dev), dy.to(dev))
    old = layers.USE_HIP_GRU
    try:
        layers.USE_HIP_GRU = False
        miopen = _grads(layer, x.to(dev), dy.to(dev))
    finally:
        layers.USE_HIP_GRU = old
    assert set(hip) == set(ref) and ("b_hh" in ref) == live_bias_hh
    _assert_within_twice_miopen(ref, hip, miopen, (T, N, H, I, reverse))


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", [(1, 5, 32, 7), (37, 5, 32, 16), (50, 6, 64, 64), (25, 70, 96, 20),
                                     (40, 37, 128, 16), (20, 130, 256, 256)])
@pytest.mark.parametrize("reverse", [False, True])
def test_small_and_ragged_shapes_match_float64(gpu_device, T, N, H, I, reverse):
    _compare(T, N, H, I, reverse, gpu_device)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_batch_larger_than_the_cu_count_matches_float64(gpu_device, reverse):
    """More batch columns than CUs: the release rule's 2 columns per workgroup, with a ragged last workgroup."""
    n = torch.cuda.get_device_properties(gpu_device).multi_processor_count + 45
    _compare(9, n, 96, 8, reverse, gpu_device, seed=6)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", [(33, 7, 96, 12), (12, 9, 256, 40)])
@pytest.mark.parametrize("reverse", [False, True])
def test_live_bias_hh_matches_float64(gpu_device, T, N, H, I, reverse):
    """bias_hh non-zero and trainable: bhh_n inside the reset gate's product, db_hh from [dr_pre, dz_pre, dq]."""
    _compare(T, N, H, I, reverse, gpu_device, seed=2, live_bias_hh=True)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_config1_layer_matches_float64(gpu_device, reverse):
    """bench.py --config 1's layer: T = 1000, N = 64, H = 96 at the layer's own initialisation."""
    _compare(1000, 64, 96, 96, reverse, gpu_device, seed=3)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_size256_layer_matches_float64(gpu_device, reverse):
    """models.mGru_flipflop's default size at the flagship's batch: T = 800, N = 128, H = 256."""
    _compare(800, 128, 256, 256, reverse, gpu_device, seed=3)


def _calls():
    return dict(layers.gru_forward_calls)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I,reverse", [(60, 21, 96, 32, False), (60, 21, 96, 32, True), (30, 10, 256, 64, True)])
def test_inference_forward_is_bit_identical_to_training_forward(gpu_device, T, N, H, I, reverse):
    """Under torch.no_grad(), with the layer's parameters trainable as they are by default, the kernel gets NULL for
    gates and q: layers.gru_forward_calls counts that launch as "inference", the call allocates no more than gx and
    y (the activations would be another 4 T N H floats), and y is the same bits as the training-mode forward's."""
    torch.manual_seed(4)
    gru = layers.GruMod(I, H)
    layer = (layers.Reverse(gru) if reverse else gru).to(gpu_device)
    assert gru.rnn.weight_hh_l0.requires_grad and gru.rnn.weight_ih_l0.requires_grad
    x = torch.randn(T, N, I, device=gpu_device)
    assert layers.hip_gru_workspace_bytes(gru.rnn, x) > 0
    before = _calls()
    train = layer(x)
    assert train.requires_grad
    assert _calls() == dict(before, saved=before["saved"] + 1)
    with torch.no_grad():
        layer(x)                        # (the workspace and the status word exist from here on)
        torch.cuda.synchronize()
        before = _calls()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        infer = layer(x)
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
    assert _calls() == dict(before, inference=before["inference"] + 1)
    assert not infer.requires_grad
    # gx (3H) + y (H) per (t, n), rounded up by the allocator; with gates and q it would be 8 T N H floats
    assert peak < 6 * T * N * H * 4, (peak, T * N * H * 4)
    assert torch.equal(train.detach(), infer)
    for p in layer.parameters():            # grad mode on, nothing requires a gradient: the same NULL-pointer forward
        p.requires_grad_(False)
    before = _calls()
    assert torch.equal(layer(x), infer)
    assert _calls() == dict(before, inference=before["inference"] + 1)
    xg = x.clone().requires_grad_(True)     # ... and an input that does: saved again
    assert torch.equal(layer(xg).detach(), infer)
    assert _calls() == dict(before, inference=before["inference"] + 1, saved=before["saved"] + 1)


@pytest.mark.gpu
@pytest.mark.parametrize("H", [32, 96, 128])
def test_lab_geometry_columns_agree(gpu_device, H):
    """The two launch geometries at sizes <= 128 (1 or 2 batch columns per workgroup; lab switch tk_lab_gru_cols)
    agree to rounding: the forward's shuffle rounds split the matvec's sum differently."""
    torch.manual_seed(5)
    layer = layers.Reverse(layers.GruMod(24, H)).to(gpu_device)
    x = torch.randn(45, 37, 24, device=gpu_device)
    dy = torch.randn(45, 37, H, device=gpu_device)
    L = _lib.use_lab(True)
    try:
        out = {}
        for cols in (1, 2):
            L.tk_lab_gru_cols(cols)
            out[cols] = _grads(layer, x, dy)
    finally:
        L.tk_lab_gru_cols(0)
        _lib.use_lab(False)
    for k in out[1]:
        assert (out[1][k] - out[2][k]).abs().max().item() <= 1e-5 * out[1][k].abs().max().item(), k


@pytest.mark.gpu
def test_captured_forward_replays_bit_identical(gpu_device):
    torch.manual_seed(7)
    layer = layers.Serial([layers.Reverse(layers.GruMod(32, 96)), layers.GruMod(96, 256)]).to(gpu_device)
    x = torch.randn(90, 21, 32, device=gpu_device)
    assert layers.hip_gru_workspace_bytes(layer[1].rnn, torch.empty(90, 21, 96, device=gpu_device)) > 0
    strict = _lib.is_strict()
    _lib.set_strict(False)
    try:
        with torch.no_grad():
            before = _calls()
            eager = layer(x)
            assert _calls() == dict(before, inference=before["inference"] + 2)
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


@pytest.mark.gpu
def test_trained_network_end_to_end_matches_float64(gpu_device):
    """The shipped network on its own chunks: HIP scores against the float64 CPU model under the 2 x MIOpen + 2e-6
    rule.  Printed, not asserted (near-ties move with rounding): the Viterbi path positions that differ from the
    path on the fixture's scores (profiles/r12_gru_errors.txt keeps the figures)."""
    from taiyaki_amd import decode
    arrays = gru_net.load_arrays()
    signal = torch.from_numpy(arrays["signal"]).unsqueeze(2)
    with torch.no_grad():
        ref = gru_net.build_model(arrays, torch.float64)(signal.double())
        net = gru_net.build_model(arrays).to(gpu_device)
        xg = signal.to(gpu_device)
        assert layers.hip_gru_workspace_bytes(net[2].rnn, torch.empty(500, 16, 96, device=gpu_device)) > 0
        hip = net(xg)
        old = layers.USE_HIP_GRU
        try:
            layers.USE_HIP_GRU = False
            miopen = net(xg)
        finally:
            layers.USE_HIP_GRU = old
        assert hip.shape == (500, 16, 40)
        _assert_within_twice_miopen({"scores": ref}, {"scores": hip}, {"scores": miopen}, "trained network")
        want = decode.flipflop_viterbi(torch.from_numpy(arrays["scores"]).to(gpu_device))[2]
        for name, sc in (("hip", hip), ("miopen", miopen)):
            path = decode.flipflop_viterbi(sc.contiguous())[2]
            print("trained network %s: max-abs against the fixture's fp32 CPU scores %.3g, Viterbi path positions "
                  "that differ %d of %d" % (name, (sc.cpu() - torch.from_numpy(arrays["scores"])).abs().max().item(),
                                            int((path != want).sum()), path.numel()))
