"""The narrow Convolution layers as fused HIP kernels (csrc/conv_kernels.hip, layers.SmallConvolution).

GPU: y, dx, dW, db against nn.Conv1d + swish evaluated in float64 on the CPU.  The tolerance is the parent path's
own error, not a constant: the unfold + GEMM evaluation (layers.USE_HIP_CONV = False) is compared with the same
float64 result, and the HIP operator's maximum error (scaled by the float64 result's largest magnitude) must be
at most twice that.  Then run-to-run and captured-replay bit identity, and independence of the workspace's contents.
CPU: which shapes are built, argument validation before any HIP call, the workspace against the slab count, and the
layer on CPU tensors.
"""
import ctypes

import pytest
import torch
from torch import nn

from taiyaki_amd import _lib, layers

SHAPES = [(1, 4, 5), (4, 16, 5)]
# (T, N): the flagship's, then tails and halos (T around the window and the tile rows, N around the wave's columns)
CASES = [(4000, 128)] + [(t, n) for t in (1, 2, 4, 5, 6, 257) for n in (1, 63, 65, 100)]


def _layer(cin, cout, k, seed):
    torch.manual_seed(seed)
    return layers.Convolution(cin, cout, k, stride=1, fun=layers.swish)


def _float64(conv, x, dy, want_dx):
    """nn.Conv1d + swish in float64 on the CPU: y, dx (or None), dW, db."""
    ref = nn.Conv1d(conv.conv.in_channels, conv.conv.out_channels, conv.winlen).double()
    with torch.no_grad():
        ref.weight.copy_(conv.conv.weight.double())
        ref.bias.copy_(conv.conv.bias.double())
    xd = x.double().requires_grad_(want_dx)
    z = ref(nn.functional.pad(xd.permute(1, 2, 0), (conv.winlen // 2, (conv.winlen - 1) // 2))).permute(2, 0, 1)
    y = z * torch.sigmoid(z)
    y.backward(dy.double())
    return y.detach(), xd.grad if want_dx else None, ref.weight.grad, ref.bias.grad


def _run(conv, x, dy, want_dx, hip):
    layers.USE_HIP_CONV = hip
    try:
        conv.zero_grad(set_to_none=True)
        xg = x.clone().requires_grad_(want_dx)
        y = conv(xg)
        y.backward(dy)
        torch.cuda.synchronize()
        return y.detach(), xg.grad if want_dx else None, conv.conv.weight.grad.clone(), conv.conv.bias.grad.clone()
    finally:
        layers.USE_HIP_CONV = True


def _err(got, want):
    return float((got.double().cpu() - want).abs().max() / want.abs().max().clamp_min(1e-300))


# conv 1 with and without an input gradient (the model's first layer has none), conv 2 with
LAYER_CASES = [((1, 4, 5), True), ((1, 4, 5), False), ((4, 16, 5), True)]


@pytest.mark.gpu
@pytest.mark.parametrize("tn", CASES, ids=lambda tn: "T%d-N%d" % tn)
@pytest.mark.parametrize("shape,want_dx", LAYER_CASES, ids=lambda v: "%dto%d" % v[:2] if isinstance(v, tuple) else "dx%d" % v)
def test_hip_convolution_is_as_close_to_float64_as_the_gemm_path(gpu_device, shape, want_dx, tn):
    cin, cout, k = shape
    (T, N) = tn
    conv = _layer(cin, cout, k, 3)
    g = torch.Generator().manual_seed(T * 1000 + N)
    x, dy = torch.randn(T, N, cin, generator=g), torch.randn(T, N, cout, generator=g)
    want = _float64(conv, x, dy, want_dx)
    conv = conv.to(gpu_device)
    x, dy = x.to(gpu_device), dy.to(gpu_device)
    hip = _run(conv, x, dy, want_dx, True)
    gemm = _run(conv, x, dy, want_dx, False)
    for name, h, p, w in zip(("y", "dx", "dW", "db"), hip, gemm, want):
        if w is None:
            assert h is None
            continue
        assert torch.isfinite(h).all(), name
        eh, ep = _err(h, w), _err(p, w)
        print("conv %d->%d T=%d N=%d dx=%d %s: hip %.3e gemm %.3e" % (cin, cout, T, N, want_dx, name, eh, ep))
        assert eh <= 2 * ep, (name, eh, ep)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dto%d" % s[:2])
def test_two_runs_and_a_replayed_forward_are_bit_identical(gpu_device, shape):
    cin, cout, k = shape
    conv = _layer(cin, cout, k, 5).to(gpu_device)
    g = torch.Generator().manual_seed(9)
    x = torch.randn(1000, 100, cin, generator=g).to(gpu_device)
    dy = torch.randn(1000, 100, cout, generator=g).to(gpu_device)
    a = _run(conv, x, dy, True, True)
    b = _run(conv, x, dy, True, True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    # captured and replayed forward (what the train step does) == eager
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side), torch.no_grad():
        conv(x)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.no_grad(), torch.cuda.graph(graph):
        yg = conv(x)
    yg.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(yg, a[0])


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dto%d" % s[:2])
def test_results_do_not_depend_on_what_the_workspace_held(gpu_device, shape):
    cin, cout, k = shape
    conv = _layer(cin, cout, k, 7).to(gpu_device)
    g = torch.Generator().manual_seed(10)
    x = torch.randn(4000, 128, cin, generator=g).to(gpu_device)
    dy = torch.randn(4000, 128, cout, generator=g).to(gpu_device)
    a = _run(conv, x, dy, True, True)
    wsb = _lib.lib().tk_conv1d_small_workspace_bytes(4000, 128, cin, cout, k, layers._cu_count(gpu_device))
    ws = _lib.workspace(wsb, gpu_device, "conv")
    assert ws.numel() >= wsb > 0
    ws.view(torch.float32)[:wsb // 4].fill_(float("nan"))
    b = _run(conv, x, dy, True, True)
    for u, v in zip(a, b):
        assert torch.equal(u, v)


@pytest.mark.gpu
def test_input_buffer_may_be_reloaded_in_place_before_backward(gpu_device):
    """The captured train step copies the next batch into the network's input buffer and replays the forward; the
    backward of the layer that read that buffer must neither be refused by autograd nor see the new values."""
    conv = _layer(1, 4, 5, 13).to(gpu_device)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(300, 7, 1, generator=g).to(gpu_device)
    dy = torch.randn(300, 7, 4, generator=g).to(gpu_device)
    want = _run(conv, x, dy, False, True)
    conv.zero_grad(set_to_none=True)
    buf = x.clone()
    y = conv(buf)
    buf.copy_(torch.randn_like(buf))
    y.backward(dy)
    assert torch.equal(conv.conv.weight.grad, want[2]) and torch.equal(conv.conv.bias.grad, want[3])


# ---------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------
def test_supported_is_exactly_the_two_narrow_layers():
    L = _lib.lib()
    yes = {(1, 4, 5, 1), (4, 16, 5, 1)}
    for cin in (1, 2, 4, 16):
        for cout in (4, 8, 16, 96, 256):
            for k in (3, 4, 5, 19):
                for stride in (1, 2, 5):
                    assert bool(L.tk_conv1d_small_supported(cin, cout, k, stride)) == ((cin, cout, k, stride) in yes)
    for no in [(16, 256, 19, 5), (1, 96, 19, 2), (1, 4, 5, 2), (4, 16, 5, 2), (1, 4, 4, 1), (4, 16, 4, 1)]:
        assert not L.tk_conv1d_small_supported(*no), no


def test_bad_arguments_are_refused_before_any_hip_call():
    L = _lib.lib()
    buf = (ctypes.c_float * 64)()
    p = ctypes.cast(buf, ctypes.c_void_p)
    odd = ctypes.c_void_p(p.value + 4)
    BAD, UNSUPPORTED, WORKSPACE = 1, 2, 3
    fwd, bwd = L.tk_conv1d_small_forward_dev, L.tk_conv1d_small_backward_dev
    assert fwd(None, p, p, 2, 2, 1, 4, 5, 256, p, None) == BAD
    assert fwd(p, None, p, 2, 2, 1, 4, 5, 256, p, None) == BAD
    assert fwd(p, p, None, 2, 2, 1, 4, 5, 256, p, None) == BAD
    assert fwd(p, p, p, 2, 2, 1, 4, 5, 256, None, None) == BAD
    assert fwd(odd, p, p, 2, 2, 1, 4, 5, 256, p, None) == BAD
    assert fwd(p, p, p, 2, 2, 1, 4, 5, 256, odd, None) == BAD
    assert fwd(p, p, p, 2, 2, 1, 4, 5, 0, p, None) == BAD
    assert fwd(p, p, p, 2, 2, 16, 256, 19, 256, p, None) == UNSUPPORTED
    assert fwd(p, p, p, 2 ** 31, 2 ** 31, 1, 4, 5, 256, p, None) == UNSUPPORTED
    ok = [p, p, p, p, 2, 2, 1, 4, 5, 256, p, p, p, p, 1 << 20, None]
    for i in (0, 1, 2, 3, 11, 12, 13):          # dy, x, weight, bias, dweight, dbias, workspace
        args = list(ok)
        args[i] = None
        assert bwd(*args) == BAD, i
    for i in (0, 1, 10, 13):                    # dy, x, dx, workspace misaligned
        args = list(ok)
        args[i] = odd
        assert bwd(*args) == BAD, i
    assert bwd(*(ok[:9] + [0] + ok[10:])) == BAD
    assert bwd(*(ok[:4] + [0, 2] + ok[6:])) == BAD
    assert bwd(*(ok[:6] + [4, 16, 4] + ok[9:])) == UNSUPPORTED
    assert bwd(*(ok[:14] + [8, None])) == WORKSPACE
    assert L.tk_conv1d_small_workspace_bytes(4000, 128, 16, 256, 19, 256) == 0
    assert L.tk_conv1d_small_workspace_bytes(0, 128, 1, 4, 5, 256) == 0
    assert L.tk_conv1d_small_workspace_bytes(4000, 128, 1, 4, 5, 0) == 0


def test_workspace_covers_one_slab_per_workgroup():
    """Tiles are 16 time rows (the winlen - 1 halo rows included when dx is wanted) by 64 / (Cout / 2) columns; the
    grid is min(tiles, 2 per CU) and every workgroup writes one slab of Cout (Cin winlen + 1) doubles."""
    L = _lib.lib()
    for cin, cout, k in SHAPES:
        cols = 64 // (cout // 2)
        slab = cout * (cin * k + 1) * 8
        for cus in (8, 16, 64, 104, 128, 228, 256, 304):
            for T, N in [(1, 1), (5, 63), (12, 16), (13, 17), (257, 100), (4000, 128), (8000, 64), (20000, 512)]:
                tiles = -(-T // (16 - (k - 1))) * -(-N // cols)
                assert tiles >= -(-T // 16) * -(-N // cols)           # (the launch without dx never has more)
                assert L.tk_conv1d_small_workspace_bytes(T, N, cin, cout, k, cus) == min(tiles, 2 * cus) * slab


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dto%d" % s[:2])
def test_convolution_on_cpu_tensors_keeps_the_gemm_path(shape, monkeypatch):
    cin, cout, k = shape
    conv = _layer(cin, cout, k, 11)
    monkeypatch.setattr(layers.SmallConvolution, "apply", None)     # (calling it would raise)
    x = torch.randn(40, 3, cin)
    y = conv(x)
    want = layers.swish(conv.conv(conv.pad(x.permute(1, 2, 0)))).permute(2, 0, 1)
    assert torch.allclose(y, want, atol=1e-6)
    conv.use_gemm = False
    assert torch.equal(conv(x), want)
