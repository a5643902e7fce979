"""The LSTM layer's parameter gradients in one pass over dG (csrc/lstm_wgrad.hip, include/taiyaki_amd_lstm_wgrad.h)
against float64 on the host, with the two GEMMs and the sum they replace (layers.LstmRecurrence.backward with
layers.USE_HIP_LSTM_WGRAD off) as the yardstick: the criterion of tests/test_lstm_hip.py, the error relative to the
largest reference entry at most twice the GEMM path's on the same device inputs, plus 2e-6."""
import ctypes
import functools
import os

import pytest
import torch

from taiyaki_amd import _lib, layers

CUS = 256
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3


def _plan(W, T, N, H, I, cus=CUS):
    out = (ctypes.c_size_t * 8)()
    if not W.tk_lab_lstm_wgrad_plan(T, N, H, I, cus, out):
        return None
    return dict(zip(("tiles_m", "tiles_n", "runs", "parts", "run_rows", "part_rows", "grid", "slabs"), out))


def test_plan_and_workspace_arithmetic(labenv):
    """The launch plan is a function of (T, N, H, I, cu_count): tiles x runs fill the CUs and never exceed them, the
    runs are whole 16-row blocks that cover the T N rows with none empty, no chain is longer than 8192 rows, and the
    workspace is one partial result [4H][I + H] | [4H] per (run, part)."""
    labenv.lib()
    W = _lib.wgrad_lib()
    assert _lib.is_lab() and set(_lib.WGRAD_LAB_SIGNATURES) == {"tk_lab_lstm_wgrad_splits", "tk_lab_lstm_wgrad_plan",
                                                                "tk_lab_lstm_wgrad_loads"}
    flagship = _plan(W, 800, 128, 256, 256)
    assert flagship == dict(tiles_m=8, tiles_n=4, runs=8, parts=2, run_rows=12800, part_rows=6400, grid=256, slabs=16)
    assert W.tk_lstm_weight_grad_workspace_bytes(800, 128, 256, 256, CUS) == 16 * (1024 * 512 + 1024) * 4
    for T, N, H, I, cus in [(1, 5, 16, 7, 256), (2, 3, 16, 1, 256), (37, 5, 16, 16, 256), (25, 70, 32, 20, 256),
                            (20, 130, 256, 256, 256), (20, 13, 64, 64, 256), (800, 128, 256, 256, 304),
                            (800, 128, 256, 256, 8), (4000, 128, 128, 16, 256), (100000, 8, 64, 300, 64)]:
        p, K = _plan(W, T, N, H, I, cus), T * N
        tiles = p["tiles_m"] * p["tiles_n"]
        assert p["tiles_m"] == -(-4 * H // 128) and p["tiles_n"] == -(-I // 128) + -(-H // 128)
        assert tiles * p["runs"] <= max(cus, tiles) and p["grid"] >= tiles * p["runs"] and p["grid"] % 8 == 0
        assert p["run_rows"] % 16 == 0 and p["part_rows"] % 16 == 0 and p["part_rows"] <= 8192
        assert (p["runs"] - 1) * p["run_rows"] < K <= p["runs"] * p["run_rows"]
        assert p["parts"] * p["part_rows"] >= p["run_rows"] and p["slabs"] == p["runs"] * p["parts"]
        slab = -(-(4 * H * (I + H) + 4 * H) // 4) * 4
        assert W.tk_lstm_weight_grad_workspace_bytes(T, N, H, I, cus) == p["slabs"] * slab * 4
    # the release library plans the same (it has no hook to say otherwise)
    R = ctypes.CDLL(os.path.join(_lib.CSRC, _lib.WGRAD_LIBNAME))
    R.tk_lstm_weight_grad_workspace_bytes.restype = ctypes.c_size_t
    R.tk_lstm_weight_grad_workspace_bytes.argtypes = [ctypes.c_size_t] * 4 + [ctypes.c_int]
    assert R.tk_lstm_weight_grad_workspace_bytes(800, 128, 256, 256, CUS) == 16 * (1024 * 512 + 1024) * 4
    assert not hasattr(R, "tk_lab_lstm_wgrad_splits")
    for shape in [(0, 5, 16, 7), (3, 0, 16, 7), (3, 5, 0, 7), (3, 5, 16, 0), (1 << 20, 1 << 12, 16, 16)]:
        assert W.tk_lstm_weight_grad_workspace_bytes(*shape, CUS) == 0, shape
    assert W.tk_lstm_weight_grad_workspace_bytes(3, 5, 16, 7, 0) == 0
    # the hook: the rows are cut into that many runs, as far as whole blocks go (260 rows are 17 blocks: 7 runs -> 6 of 3)
    try:
        got = []
        for splits in (1, 2, 3, 7):
            W.tk_lab_lstm_wgrad_splits(splits)
            p = _plan(W, 20, 13, 64, 64)
            got.append((p["runs"], p["run_rows"]))
        assert got == [(1, 272), (2, 144), (3, 96), (6, 48)]
    finally:
        W.tk_lab_lstm_wgrad_splits(0)


def test_bad_arguments_are_refused_before_any_launch():
    """NULL -> TK_ERR_BAD_ARG, a workspace one byte short -> TK_ERR_WORKSPACE, a shape with no plan ->
    TK_ERR_UNSUPPORTED: decided on the host (the pointers here are never dereferenced: there is no GPU in this test)."""
    W = _lib.wgrad_lib()
    T, N, H, I = 37, 5, 16, 16
    need = W.tk_lstm_weight_grad_workspace_bytes(T, N, H, I, CUS)
    assert need > 0
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(7)]     # dgates, x, y, dw_ih, dw_hh, db, workspace

    def call(ptrs, wsb, shape=(T, N, H, I)):
        return W.tk_lstm_weight_grad_dev(ptrs[0], ptrs[1], ptrs[2], *shape, 0, CUS, ptrs[3], ptrs[4], ptrs[5], ptrs[6],
                                         wsb, None)

    for i in range(7):
        assert call(p[:i] + [ctypes.c_void_p(0)] + p[i + 1:], need) == BAD_ARG, i
    assert call(p[:6] + [ctypes.c_void_p(4096 + 4)], need) == BAD_ARG       # the workspace is 16-byte aligned
    assert call(p, need - 1) == WORKSPACE
    assert call(p, 0) == WORKSPACE
    assert call(p, need, (0, N, H, I)) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def _case(T, N, H, I):
    """dG, x, y (float32, host) with the first and the last time step at 50 x the rest -- a dropped or doubled boundary
    row, or a shift the wrong way, is then a gross error -- and the float64 results for both directions."""
    g = torch.Generator().manual_seed(1000 * T + 10 * N + H + I)
    dg, x, y = (torch.randn(T, N, C, generator=g) for C in (4 * H, I, H))
    for t in (dg, x, y):
        t[0] *= 50
        t[-1] *= 50
    d = dg.double().reshape(T * N, 4 * H)
    ref = {}
    for reverse in (False, True):
        if T > 1:
            ds, hp = (dg[:-1], y[1:]) if reverse else (dg[1:], y[:-1])
            w_hh = ds.double().reshape(-1, 4 * H).t() @ hp.double().reshape(-1, H)
        else:
            w_hh = torch.zeros(4 * H, H, dtype=torch.float64)
        ref[reverse] = dict(w_ih=d.t() @ x.double().reshape(T * N, I), w_hh=w_hh, b=d.sum(0))
    return dg, x, y, ref


def _gemms(dg, x, y, reverse):
    """The three lines of LstmRecurrence.backward that the kernel replaces, on the device tensors."""
    T, N, H = y.shape
    dg2 = dg.view(T * N, 4 * H)
    if T > 1:
        dgs, hp = (dg[:-1], y[1:]) if reverse else (dg[1:], y[:-1])
        w_hh = dgs.reshape(-1, 4 * H).t() @ hp.reshape(-1, H)
    else:
        w_hh = torch.zeros(4 * H, H, device=dg.device)
    return dict(w_ih=dg2.t() @ x.view(T * N, -1), w_hh=w_hh, b=dg2.sum(0))


def _kernel(W, dg, x, y, reverse, poison=None):
    T, N, H = y.shape
    I = x.shape[2]
    dev = dg.device
    wsb = W.tk_lstm_weight_grad_workspace_bytes(T, N, H, I, CUS)
    assert wsb > 0
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    if poison is not None:
        ws.fill_(poison)
    out = dict(w_ih=torch.full((4 * H, I), float("nan"), device=dev), w_hh=torch.full((4 * H, H), float("nan"), device=dev),
               b=torch.full((4 * H,), float("nan"), device=dev))
    rc = W.tk_lstm_weight_grad_dev(_lib.ptr(dg), _lib.ptr(x), _lib.ptr(y), T, N, H, I, int(reverse), CUS,
                                   _lib.ptr(out["w_ih"]), _lib.ptr(out["w_hh"]), _lib.ptr(out["b"]), _lib.ptr(ws), wsb,
                                   _lib.stream_ptr())
    assert rc == OK
    torch.cuda.synchronize()
    return out


def _errors(got, ref):
    return {k: (got[k].double().cpu() - r).abs().max().item() / (r.abs().max().item() or 1.0) for k, r in ref.items()}


def _check(T, N, H, I, dev, W):
    dg, x, y, ref = _case(T, N, H, I)
    dg, x, y = dg.to(dev), x.to(dev), y.to(dev)
    outs = {}
    for reverse in (False, True):
        e_gemm = _errors(_gemms(dg, x, y, reverse), ref[reverse])
        outs[reverse] = _kernel(W, dg, x, y, reverse)
        e_hip = _errors(outs[reverse], ref[reverse])
        print("wgrad (T, N, H, I) = %s reverse %d: kernel %s, GEMMs %s" % ((T, N, H, I), reverse, e_hip, e_gemm))
        for k in e_hip:
            assert e_hip[k] <= 2 * e_gemm[k] + 2e-6, (T, N, H, I, reverse, k, e_hip[k], e_gemm[k])
        if T == 1:
            assert outs[reverse]["w_hh"].abs().max().item() == 0.0
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", [(1, 5, 16, 7), (2, 3, 16, 1), (37, 5, 16, 16), (25, 70, 32, 20), (20, 130, 256, 256)])
def test_kernel_matches_float64_as_the_gemms_do(gpu_device, T, N, H, I):
    """K smaller than one block and dW_hh exactly zero; one shifted pair and I = 1; a ragged last block and an output
    smaller than a tile; ragged I and N; the full 1024 x 513 output, several tiles each way."""
    _check(T, N, H, I, gpu_device, _lib.wgrad_lib())


@pytest.mark.gpu
def test_forced_runs_agree_and_match_float64(gpu_device, labenv):
    """(20, 13, 64, 64) cut into 1, 2, 3 and 7 runs (realised as 1, 2, 3 and 6: test_plan_and_workspace_arithmetic):
    the boundaries, multiples of 16 rows, fall inside time steps of 13 rows and the shifted read of y crosses them."""
    labenv.lib()
    W = _lib.wgrad_lib()
    T, N, H, I = 20, 13, 64, 64
    ref = _case(T, N, H, I)[3]
    dg, x, y = (t.to(gpu_device) for t in _case(T, N, H, I)[:3])
    outs = []
    try:
        for splits in (1, 2, 3, 7):
            W.tk_lab_lstm_wgrad_splits(splits)
            outs.append(_check(T, N, H, I, gpu_device, W))
    finally:
        W.tk_lab_lstm_wgrad_splits(0)
    for reverse in (False, True):
        e_gemm = _errors(_gemms(dg, x, y, reverse), ref[reverse])
        for i in range(len(outs)):
            for j in range(i):
                for k, r in ref[reverse].items():
                    diff = (outs[i][reverse][k] - outs[j][reverse][k]).abs().max().item() / r.abs().max().item()
                    assert diff <= 2 * e_gemm[k] + 2e-6, (i, j, reverse, k, diff)


@pytest.mark.gpu
def test_two_calls_are_bit_identical(gpu_device):
    """... whatever the workspace held before either."""
    W = _lib.wgrad_lib()
    dg, x, y = (t.to(gpu_device) for t in _case(20, 130, 256, 256)[:3])
    for reverse in (False, True):
        a = _kernel(W, dg, x, y, reverse, poison=float("nan"))
        b = _kernel(W, dg, x, y, reverse, poison=3.0)
        for k in a:
            assert torch.equal(a[k], b[k]), (reverse, k)


def _layer_grads(layer, x, dy, switch):
    old = layers.USE_HIP_LSTM_WGRAD
    layers.USE_HIP_LSTM_WGRAD = switch
    try:
        x = x.detach().clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        y = layer(x)
        (y * dy).sum().backward()
    finally:
        layers.USE_HIP_LSTM_WGRAD = old
    rnn = layer.layer.rnn if isinstance(layer, layers.Reverse) else layer.rnn
    out = {"y": y, "x": x.grad, "w_ih": rnn.weight_ih_l0.grad, "w_hh": rnn.weight_hh_l0.grad, "b_ih": rnn.bias_ih_l0.grad}
    return {k: v.detach().clone() for k, v in out.items()}


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", [(20, 130, 256, 256), (37, 5, 16, 7)])
@pytest.mark.parametrize("reverse", [False, True])
def test_through_the_layer_with_the_switch_on_and_off(gpu_device, T, N, H, I, reverse):
    torch.manual_seed(11)
    lstm = layers.Lstm(I, H)
    layer = layers.Reverse(lstm) if reverse else lstm
    x = torch.randn(T, N, I)
    dy = torch.randn(T, N, H) / (T * N) ** 0.5
    ref = _layer_grads(layer.double(), x.double(), dy.double(), True)
    layer = layer.float().to(gpu_device)
    assert layers.hip_lstm_workspace_bytes(lstm.rnn, x.to(gpu_device)) > 0
    on = _layer_grads(layer, x.to(gpu_device), dy.to(gpu_device), True)
    off = _layer_grads(layer, x.to(gpu_device), dy.to(gpu_device), False)
    assert torch.equal(on["y"], off["y"]) and torch.equal(on["x"], off["x"])
    for k in ("w_ih", "w_hh", "b_ih"):
        scale = ref[k].abs().max().item()
        e_on = (on[k].double().cpu() - ref[k]).abs().max().item() / scale
        e_off = (off[k].double().cpu() - ref[k]).abs().max().item() / scale
        print("layer (T, N, H, I) = %s reverse %d %s: kernel %.3g, GEMMs %.3g" % ((T, N, H, I), reverse, k, e_on, e_off))
        assert e_on <= 2 * e_off + 2e-6, (k, e_on, e_off)


@pytest.mark.gpu
def test_refusals_leave_the_outputs_alone(gpu_device):
    """A workspace one byte too small returns TK_ERR_WORKSPACE, a NULL pointer TK_ERR_BAD_ARG, and nothing is launched:
    the outputs keep what they held."""
    W = _lib.wgrad_lib()
    T, N, H, I = 37, 5, 16, 16
    dg, x, y = (t.to(gpu_device) for t in _case(T, N, H, I)[:3])
    wsb = W.tk_lstm_weight_grad_workspace_bytes(T, N, H, I, CUS)
    ws = torch.full((wsb // 4,), 7.0, device=gpu_device)
    outs = [torch.full(s, 7.0, device=gpu_device) for s in ((4 * H, I), (4 * H, H), (4 * H,))]

    def call(dgp, wsbytes):
        return W.tk_lstm_weight_grad_dev(dgp, _lib.ptr(x), _lib.ptr(y), T, N, H, I, 0, CUS, _lib.ptr(outs[0]),
                                         _lib.ptr(outs[1]), _lib.ptr(outs[2]), _lib.ptr(ws), wsbytes, _lib.stream_ptr())

    assert call(_lib.ptr(dg), wsb - 1) == WORKSPACE
    assert call(_lib.ptr(None), wsb) == BAD_ARG
    torch.cuda.synchronize()
    assert all(bool((t == 7.0).all()) for t in outs + [ws])
