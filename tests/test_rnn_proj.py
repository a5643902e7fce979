"""The recurrent layers' two projection GEMMs on split bf16 operands (csrc/rnn_proj.hip, include/taiyaki_amd_rnn_proj.h)
against float64 on the host, with the rocBLAS call each replaces (torch.addmm, `@`) as the yardstick: the criterion of
tests/test_lstm_wgrad.py and tests/test_lstm_split_gemm.py, the error relative to the largest reference entry at most
twice the GEMM's on the same device tensors, plus 2e-6.  The shapes are the smallest at which the kernel can go wrong:
rows around its 128-row tile, every pair of widths of the rule's ends and the flagship's widths at a few rows."""
import ctypes
import functools
import os

import pytest
import torch

from taiyaki_amd import _lib, layers

CUS = 256
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
RT, NT, KB = 128, 128, 16       # the kernel's tile: rows, columns, k per block (csrc/rnn_proj.hip)
B_BLOCK = 3 * 4 * 1024          # bytes of the three B images of one (column tile, k block)
WIDTHS = (16, 32, 64, 96, 128, 192, 256, 384)
GRAD_MIN_ROWS = 64000          # the gradient form (k > nout) is admitted from here on


def _plan_py(rows, k, nout):
    """The tile rule restated: None where the kernel does not run."""
    lo, hi = min(k, nout), max(k, nout)
    if rows == 0 or lo not in WIDTHS or hi not in (3 * lo, 4 * lo) or rows >= (1 << 31) // hi:
        return None
    if k > nout and rows < GRAD_MIN_ROWS:
        return None
    tm, tn, nkb = -(-rows // RT), -(-nout // NT), -(-k // KB)
    return dict(rt=RT, nt=NT, tiles_m=tm, tiles_n=tn, nkb=nkb, grid=-(-tm // 8) * 8 * tn)


def _plan(P, rows, k, nout, cus=CUS):
    out = (ctypes.c_size_t * 6)()
    if not P.tk_lab_rnn_proj_plan(rows, k, nout, cus, out):
        return None
    return dict(zip(("rt", "nt", "tiles_m", "tiles_n", "nkb", "grid"), out))


def test_header_parses_into_the_binding():
    assert set(_lib.RNN_PROJ_SIGNATURES) == {"tk_rnn_proj_workspace_bytes", "tk_rnn_input_proj_dev",
                                             "tk_rnn_input_grad_dev"}
    assert set(_lib.RNN_PROJ_LAB_SIGNATURES) == {"tk_lab_rnn_proj_plan"}
    res, args = _lib.RNN_PROJ_SIGNATURES["tk_rnn_proj_workspace_bytes"]
    assert res is ctypes.c_size_t and args == [ctypes.c_size_t] * 3 + [ctypes.c_int]
    res, args = _lib.RNN_PROJ_SIGNATURES["tk_rnn_input_proj_dev"]
    assert res is ctypes.c_int and len(args) == 11 and args[:3] == [ctypes.c_void_p] * 3
    assert len(_lib.RNN_PROJ_SIGNATURES["tk_rnn_input_grad_dev"][1]) == 10
    P = _lib.rnn_proj_lib()         # every symbol resolves
    assert not hasattr(P, "tk_lab_rnn_proj_plan") or _lib.is_lab()


def test_workspace_rule():
    """0 for a zero size, for widths outside the rule, for rows x width beyond 32-bit indexing and for the gradient form
    below 64000 rows; positive at the flagship; a function of its arguments only -- the projection form's not of rows
    or the CU count at all."""
    P = _lib.rnn_proj_lib()
    ws = P.tk_rnn_proj_workspace_bytes
    assert ws(800 * 128, 256, 1024, CUS) == 8 * 16 * B_BLOCK
    assert ws(800 * 128, 1024, 256, CUS) == 2 * 64 * B_BLOCK
    for shape in [(0, 256, 1024), (5, 0, 1024), (5, 256, 0)]:
        assert ws(*shape, CUS) == 0, shape
    assert ws(5, 256, 1024, 0) == 0
    for k, nout in [(256, 512), (256, 256), (100, 400), (24, 96), (512, 2048), (8, 32), (256, 1280), (255, 1020)]:
        assert ws(5, k, nout, CUS) == 0 and ws(5, nout, k, CUS) == 0, (k, nout)
    for H in WIDTHS:
        for gates in (3, 4):
            want = -(-gates * H // NT) * -(-H // KB) * B_BLOCK
            assert ws(7, H, gates * H, CUS) == want, (H, gates)
            assert ws(7, gates * H, H, CUS) == 0 and ws(GRAD_MIN_ROWS - 1, gates * H, H, CUS) == 0
            assert ws(GRAD_MIN_ROWS, gates * H, H, CUS) == -(-H // NT) * -(-gates * H // KB) * B_BLOCK
    assert ws((1 << 31) // 1024 - 1, 256, 1024, CUS) > 0
    assert ws((1 << 31) // 1024, 256, 1024, CUS) == 0 and ws((1 << 31) // 1024, 1024, 256, CUS) == 0
    assert ws(1 << 40, 16, 64, CUS) == 0
    for rows in (1, 127, 128, 129, 100000):
        for cus in (1, 8, 256, 304):
            assert ws(rows, 256, 1024, cus) == ws(1, 256, 1024, CUS)
            assert ws(rows, 96, 288, cus) == ws(1, 96, 288, CUS)
    for rows in (GRAD_MIN_ROWS, 100000, 1 << 20):
        for cus in (1, 256, 304):
            assert ws(rows, 1024, 256, cus) == ws(GRAD_MIN_ROWS, 1024, 256, CUS) > 0
            assert ws(rows, 288, 96, cus) == ws(GRAD_MIN_ROWS, 288, 96, CUS) > 0


def test_plan_hook_agrees_with_the_python_rule(labenv):
    labenv.lib()
    P = _lib.rnn_proj_lib()
    assert _lib.is_lab()
    assert _plan(P, 800 * 128, 256, 1024) == dict(rt=128, nt=128, tiles_m=800, tiles_n=8, nkb=16, grid=6400)
    for rows in (1, RT - 1, RT, RT + 1, 8 * RT, 8 * RT + 1, 2 * RT + 3, GRAD_MIN_ROWS - 1, GRAD_MIN_ROWS, 800 * 128):
        for k, nout in [(16, 64), (64, 16), (16, 48), (48, 16), (32, 128), (128, 32), (96, 288), (288, 96), (128, 384),
                        (192, 768), (256, 1024), (1024, 256), (384, 1536), (1536, 384), (384, 1152), (100, 400)]:
            assert _plan(P, rows, k, nout) == _plan_py(rows, k, nout), (rows, k, nout)
            want = _plan_py(rows, k, nout)
            assert P.tk_rnn_proj_workspace_bytes(rows, k, nout, CUS) == (want["tiles_n"] * want["nkb"] * B_BLOCK if want else 0)
    assert _plan(P, (1 << 31) // 1536, 384, 1536) is None and _plan(P, (1 << 31) // 1536 - 1, 384, 1536) is not None


def test_bad_arguments_are_refused_before_any_launch():
    """NULL or a misaligned workspace -> TK_ERR_BAD_ARG, a workspace one byte short -> TK_ERR_WORKSPACE, widths outside
    the rule -> TK_ERR_UNSUPPORTED: decided on the host (the pointers are never dereferenced: no GPU in this test)."""
    P = _lib.rnn_proj_lib()
    need = P.tk_rnn_proj_workspace_bytes(33, 16, 64, CUS)
    assert need > 0
    a, w, b, out, ws = (ctypes.c_void_p(4096 * (i + 1)) for i in range(5))
    null = ctypes.c_void_p(0)

    def proj(a=a, w=w, out=out, ws=ws, wsb=need, shape=(33, 16, 64)):
        return P.tk_rnn_input_proj_dev(a, w, b, *shape, CUS, out, ws, wsb, None)

    def grad(a=a, w=w, out=out, ws=ws, wsb=need, shape=(33, 16, 64)):
        return P.tk_rnn_input_grad_dev(a, w, *shape, CUS, out, ws, wsb, None)

    for call in (proj, grad):
        for name in ("a", "w", "out", "ws"):
            assert call(**{name: null}) == BAD_ARG, name
        assert call(ws=ctypes.c_void_p(4096 + 4)) == BAD_ARG
        assert call(wsb=need - 1) == WORKSPACE and call(wsb=0) == WORKSPACE
        assert call(shape=(0, 16, 64)) == UNSUPPORTED and call(shape=(33, 16, 32)) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------
GUARD = 64


def _run(a, w, bias, grad, poison=0xFF, out_shift=0):
    """One call on device tensors: a (M, K), w = W_ih (G, I), bias (G) or None.  The output lies between two guard
    bands over a sentinel and the workspace is poisoned; returns the output (M, nout).  The entry points run at every
    number of rows; the workspace, which depends on the widths alone, is asked for at a number the rule admits."""
    P = _lib.rnn_proj_lib()
    M, K = a.shape
    G, I = w.shape
    nout = I if grad else G
    assert K == (G if grad else I)
    dev = a.device
    wsb = P.tk_rnn_proj_workspace_bytes(max(M, 1 << 16), K, nout, CUS)
    assert wsb > 0
    ws = torch.full((wsb,), poison, dtype=torch.uint8, device=dev)
    buf = torch.full((GUARD + out_shift + M * nout + GUARD,), 7.0, device=dev)
    out = buf[GUARD + out_shift:GUARD + out_shift + M * nout]
    out.fill_(float("nan"))
    if grad:
        rc = P.tk_rnn_input_grad_dev(_lib.ptr(a), _lib.ptr(w), M, I, G, CUS, _lib.ptr(out), _lib.ptr(ws), wsb,
                                     _lib.stream_ptr())
    else:
        rc = P.tk_rnn_input_proj_dev(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), M, I, G, CUS, _lib.ptr(out), _lib.ptr(ws),
                                     wsb, _lib.stream_ptr())
    assert rc == OK
    torch.cuda.synchronize()
    assert (buf[:GUARD + out_shift] == 7.0).all() and (buf[GUARD + out_shift + M * nout:] == 7.0).all(), "guard bands"
    return out.view(M, nout).clone()


def _gemm(a, w, bias, grad):
    if grad:
        return a @ w
    return torch.addmm(bias, a, w.t()) if bias is not None else a @ w.t()


def _ref64(a, w, bias, grad):
    r = a.double() @ (w.double() if grad else w.double().t())
    return r + bias.double() if bias is not None and not grad else r


def _rel(got, ref):
    return (got.double().cpu() - ref).abs().max().item() / (ref.abs().max().item() or 1.0)


@functools.lru_cache(maxsize=None)
def _inputs(kind, M, I, G, grad):
    """a, W_ih, bias on the host (float32) and the float64 result.  `kind`: randn; cancel (a = 1 + 2^-10 randn against
    rows of B that sum to about 0: the result is made of the correction terms); scale (a x 1e3, W x 1e-6)."""
    g = torch.Generator().manual_seed(7 * M + 3 * I + G + 1000 * grad + len(kind))
    K = G if grad else I
    a = torch.randn(M, K, generator=g)
    w = torch.randn(G, I, generator=g) / K ** 0.5
    bias = None if grad else torch.randn(G, generator=g)
    if kind == "cancel":
        a = 1 + a * 2.0 ** -10
        w = w - w.mean(0 if grad else 1, keepdim=True)     # B[n][:] sums to about 0 over k
        bias = None if grad else torch.zeros(G)
    elif kind == "scale":
        a, w = a * 1e3, w * 1e-6
        bias = None if grad else bias * 1e-3
    return a, w, bias, _ref64(a, w, bias, grad)


def _check(kind, M, I, G, grad, dev, with_bias=True):
    a, w, bias, ref = _inputs(kind, M, I, G, grad)
    if not with_bias and not grad:
        bias, ref = None, _ref64(a, w, None, grad)
    a, w = a.to(dev), w.to(dev)
    bias = bias.to(dev) if bias is not None else None
    got = _run(a, w, bias, grad)
    assert torch.isfinite(got).all(), "every element is overwritten"
    e_hip, e_gemm = _rel(got, ref), _rel(_gemm(a, w, bias, grad), ref)
    print("proj %s (M, I, G) = %s grad %d bias %d: kernel %.3g, GEMM %.3g" % (kind, (M, I, G), grad, bias is not None,
                                                                             e_hip, e_gemm))
    assert e_hip <= 2 * e_gemm + 2e-6, (kind, M, I, G, grad, e_hip, e_gemm)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("M", [1, RT - 1, RT, RT + 1, 2 * RT + 3])
def test_flagship_widths_around_the_row_tile(gpu_device, M, grad):
    """(K, Nout) = (256, 1024) and (1024, 256): no rows but one, a tile less a row, a whole tile, a row more, and three
    tiles of which the last holds three rows."""
    for kind in ("randn", "cancel", "scale"):
        _check(kind, M, 256, 1024, grad, gpu_device)
    if not grad:
        _check("randn", M, 256, 1024, grad, gpu_device, with_bias=False)


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("I,G", [(16, 64), (16, 48), (96, 288), (96, 384), (192, 768), (384, 1536), (384, 1152)])
def test_other_widths_at_33_rows(gpu_device, I, G, grad):
    """k of one block (16) and of three (48), outputs narrower than a tile and not whole tiles (288), the widest of the
    rule; both entry points, with and without a bias."""
    for kind in ("randn", "cancel", "scale"):
        _check(kind, 33, I, G, grad, gpu_device)
    if not grad:
        _check("randn", 33, I, G, grad, gpu_device, with_bias=False)


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [False, True])
def test_the_cancelling_input_cancels(gpu_device, grad):
    """... so that test's result is made of the correction terms: the largest result is below 1 % of the sum of the
    magnitudes of its products."""
    a, w, _, ref = _inputs("cancel", RT + 1, 256, 1024, grad)
    mags = a.double().abs() @ (w.double().abs() if grad else w.double().abs().t())
    assert ref.abs().max().item() < 1e-2 * mags.max().item()


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [False, True])
def test_zero_rows_give_the_bias_or_zero_as_bits(gpu_device, grad):
    M, I, G = 2 * RT + 3, 256, 1024
    a, w, bias, _ = _inputs("randn", M, I, G, grad)
    a = a.clone()
    zero = [0, 5, RT - 1, RT, M - 1]
    a[zero] = 0
    got = _run(a.to(gpu_device), w.to(gpu_device), None if grad else bias.to(gpu_device), grad).cpu()
    want = torch.zeros(len(zero), I) if grad else bias.expand(len(zero), G)
    assert torch.equal(got[zero].view(torch.int32), want.contiguous().view(torch.int32))
    clean = _run(_inputs("randn", M, I, G, grad)[0].to(gpu_device), w.to(gpu_device),
                 None if grad else bias.to(gpu_device), grad).cpu()
    rest = [m for m in range(M) if m not in zero]
    assert torch.equal(got[rest].view(torch.int32), clean[rest].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [False, True])
@pytest.mark.parametrize("I,G", [(256, 1024), (96, 288)])
def test_rows_are_independent_of_the_batch_they_are_in(gpu_device, I, G, grad):
    """Rows {0, RT - 1, RT, M - 1} of an M = 2 RT + 3 call, bit for bit, computed alone (M = 1) and at other positions
    of an M = RT call among other rows; and two calls, over differently poisoned workspaces, give equal bits."""
    M = 2 * RT + 3
    a, w, bias, _ = _inputs("randn", M, I, G, grad)
    a, w = a.to(gpu_device), w.to(gpu_device)
    bias = None if grad else bias.to(gpu_device)
    full = _run(a, w, bias, grad)
    assert torch.equal(full.view(torch.int32), _run(a, w, bias, grad, poison=0x3F).view(torch.int32))
    rows, places = [0, RT - 1, RT, M - 1], [5, 0, RT - 1, 64]
    for m in rows:
        alone = _run(a[m:m + 1].contiguous(), w, bias, grad)
        assert torch.equal(alone.view(torch.int32), full[m:m + 1].view(torch.int32)), m
    other = torch.randn(RT, a.shape[1], generator=torch.Generator().manual_seed(5)).to(gpu_device)
    other[places] = a[rows]
    moved = _run(other, w, bias, grad)
    assert torch.equal(moved[places].view(torch.int32), full[rows].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("M,I,G,grad,column_tiles", [(8 * RT + 1, 64, 256, False, 2), (8 * RT + 1, 64, 256, True, 1),
                                                     (8 * RT + 1, 192, 768, True, 2), (17 * RT, 16, 64, False, 1),
                                                     (17 * RT, 16, 64, True, 1)])
def test_row_tiles_beyond_the_first_group_of_eight(gpu_device, M, I, G, grad, column_tiles):
    """blockIdx walks the row tiles in groups of eight, the column tiles of a group inside it.  A ninth row tile of one
    row under two column tiles (the projection at (64, 256), the gradient at (192, 768)) and under one; 17 row tiles:
    three groups, the last with one tile.  Rows 0, 1023, 1024 and M - 1 are the bits of the same rows computed alone."""
    assert -(-M // RT) > 8 and -(-(I if grad else G) // NT) == column_tiles
    a, w, bias, _ = _inputs("randn", M, I, G, grad)
    full = _check("randn", M, I, G, grad, gpu_device)
    a, w = a.to(gpu_device), w.to(gpu_device)
    bias = None if grad else bias.to(gpu_device)
    for m in (0, 8 * RT - 1, 8 * RT, M - 1):
        alone = _run(a[m:m + 1].contiguous(), w, bias, grad)
        assert torch.equal(alone.view(torch.int32), full[m:m + 1].view(torch.int32)), m


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [False, True])
def test_a_non_finite_element_stays_in_its_row(gpu_device, grad):
    M, I, G = RT + 1, 96, 288
    a, w, bias, _ = _inputs("randn", M, I, G, grad)
    a, w = a.to(gpu_device), w.to(gpu_device)
    bias = None if grad else bias.to(gpu_device)
    clean = _run(a, w, bias, grad)
    bad = a.clone()
    bad[3, 7], bad[RT - 1, 0], bad[RT, a.shape[1] - 1] = float("inf"), float("nan"), float("-inf")
    got = _run(bad, w, bias, grad)
    hit = [3, RT - 1, RT]
    assert not torch.isfinite(got[hit]).any()
    rest = [m for m in range(M) if m not in hit]
    assert torch.equal(got[rest].view(torch.int32), clean[rest].view(torch.int32))


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [False, True])
def test_tensors_four_bytes_off_alignment(gpu_device, grad):
    """`a` 4 bytes off 16-byte alignment takes the guarded loads; w_ih, the bias and the output need float alignment
    only.  The arithmetic is the same: equal bits."""
    M, I, G = RT + 1, 96, 288
    a, w, bias, _ = _inputs("randn", M, I, G, grad)
    a, w = a.to(gpu_device), w.to(gpu_device)
    bias = None if grad else bias.to(gpu_device)
    want = _run(a, w, bias, grad)

    def off(t):
        flat = torch.empty(t.numel() + 4, device=gpu_device)
        shift = 1 + (-(flat.data_ptr() // 4)) % 4       # flat[shift:] starts 4 bytes past a 16-byte boundary
        v = flat[shift:shift + t.numel()].view(t.shape)
        v.copy_(t)
        assert v.data_ptr() % 16 == 4
        return v

    assert torch.equal(_run(off(a), w, bias, grad).view(torch.int32), want.view(torch.int32))
    assert torch.equal(_run(a, off(w), None if grad else off(bias), grad).view(torch.int32), want.view(torch.int32))
    assert torch.equal(_run(a, w, bias, grad, out_shift=1).view(torch.int32), want.view(torch.int32))


def _layer_run(layer, x, dy, switch):
    old = layers.USE_HIP_RNN_PROJ
    layers.USE_HIP_RNN_PROJ = switch
    try:
        x = x.detach().clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        y = layer(x)
        (y * dy).sum().backward()
    finally:
        layers.USE_HIP_RNN_PROJ = old
    rnn = layer.rnn
    out = {"y": y, "x": x.grad, "w_ih": rnn.weight_ih_l0.grad, "w_hh": rnn.weight_hh_l0.grad, "b_ih": rnn.bias_ih_l0.grad}
    return {k: v.detach().clone() for k, v in out.items()}


def _layer_on_off(layer, H, workspace_bytes, dev, T=5, N=3):
    x, dy = torch.randn(T, N, H), torch.randn(T, N, H) / (T * N) ** 0.5
    ref = _layer_run(layer.double(), x.double(), dy.double(), True)
    layer = layer.float().to(dev)
    assert workspace_bytes(layer.rnn, x.to(dev)) > 0
    gates = layer.rnn.weight_ih_l0.shape[0]
    assert _lib.rnn_proj_lib().tk_rnn_proj_workspace_bytes(T * N, H, gates, layers._cu_count(dev)) > 0
    on = _layer_run(layer, x.to(dev), dy.to(dev), True)
    off = _layer_run(layer, x.to(dev), dy.to(dev), False)
    for k, r in ref.items():
        scale = r.abs().max().item()
        d_on = (on[k] - off[k]).abs().max().item() / scale
        e_off = (off[k].double().cpu() - r).abs().max().item() / scale
        print("%s H = %d %s: kernel - rocBLAS %.3g, rocBLAS - float64 %.3g" % (type(layer).__name__, H, k, d_on, e_off))
        assert d_on <= 2 * e_off + 2e-6, (k, d_on, e_off)


@pytest.mark.gpu
@pytest.mark.parametrize("H,T,N", [(32, 5, 3), (256, 5, 3), (32, 500, 128)])
def test_through_the_layer_with_the_switch_on_and_off(gpu_device, H, T, N):
    """layers.Lstm(H, H) at T = 5, N = 3: the output and every gradient with the kernel differ from those with rocBLAS
    by at most twice what rocBLAS's differ from float64 by, plus 2e-6 (relative to the largest entry).  At 15 rows the
    input gradient stays on rocBLAS (the rule); T = 500, N = 128 are the 64000 rows from which it is the kernel's too."""
    torch.manual_seed(11)
    P, cus = _lib.rnn_proj_lib(), layers._cu_count(gpu_device)
    assert (P.tk_rnn_proj_workspace_bytes(T * N, 4 * H, H, cus) > 0) == (T * N >= GRAD_MIN_ROWS)
    _layer_on_off(layers.Lstm(H, H), H, layers.hip_lstm_workspace_bytes, gpu_device, T, N)


@pytest.mark.gpu
def test_through_the_gru_layer_with_the_switch_on_and_off(gpu_device):
    """layers.GruMod(96, 96), the size of the reference's default network, likewise."""
    torch.manual_seed(12)
    _layer_on_off(layers.GruMod(96, 96), 96, layers.hip_gru_workspace_bytes, gpu_device)


@pytest.mark.gpu
def test_captured_forward_replays_bit_identical(gpu_device):
    torch.manual_seed(7)
    layer = layers.Lstm(32, 32).to(gpu_device)
    x = torch.randn(5, 3, 32, device=gpu_device)
    assert layers.hip_lstm_workspace_bytes(layer.rnn, x) > 0
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
            out.fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            assert torch.equal(out, eager)
        _lib.raise_if_nonfinite()
    finally:
        _lib.set_strict(strict)
