"""The GRU layer's parameter gradients in one pass over dG and dq (csrc/gru_wgrad.hip, the kernel of
csrc/wgrad_common.h; include/taiyaki_amd_gru_wgrad.h) against float64 on the host, with the batched GEMMs, sums and cats
they replace (layers._gru_grads_from_dgates with layers.USE_HIP_GRU_WGRAD off) as the yardstick: the criterion of
tests/test_lstm_wgrad.py, the error relative to the largest reference entry at most twice the GEMM path's on the same
device inputs, plus 2e-6, for each of dW_ih, dW_hh, db_ih and db_hh."""
import copy
import ctypes
import functools
import os
import re
import subprocess

import pytest
import torch

from taiyaki_amd import _lib, layers

CUS = 256
OK, BAD_ARG, UNSUPPORTED, WORKSPACE = 0, 1, 2, 3
KEYS = ("w_ih", "w_hh", "b_ih", "b_hh")


def _plan(W, T, N, H, I, cus=CUS):
    out = (ctypes.c_size_t * 8)()
    if not W.tk_lab_gru_wgrad_plan(T, N, H, I, cus, out):
        return None
    return dict(zip(("tiles_m", "tiles_n", "runs", "parts", "run_rows", "part_rows", "grid", "slabs"), out))


def _exported(libname):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                         capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_the_libraries_export_what_the_header_declares():
    """nm -D of the release library is the header's functions outside TK_LAB; the lab library adds exactly the three
    tk_lab_gru_wgrad_* hooks.  The binding is read from the same header."""
    text = open(_lib.GRU_WGRAD_HEADER).read()
    lab_block = re.search(r"#ifdef TK_LAB\n(.*?)#endif", text, re.S).group(1)
    lab = set(_lib.parse_prototypes(_lib._blank_comments(lab_block)))
    public = set(_lib.parse_prototypes(_lib._blank_comments(text))) - lab
    assert public == {"tk_gru_weight_grad_workspace_bytes", "tk_gru_weight_grad_dev"}
    assert lab == {"tk_lab_gru_wgrad_splits", "tk_lab_gru_wgrad_plan", "tk_lab_gru_wgrad_loads"}
    assert _exported(_lib.GRU_WGRAD_LIBNAME) == public
    assert _exported(_lib.GRU_WGRAD_LAB_LIBNAME) == public | lab
    assert set(_lib.GRU_WGRAD_SIGNATURES) == public and set(_lib.GRU_WGRAD_LAB_SIGNATURES) == lab
    assert not _lib.is_lab() and not hasattr(_lib.gru_wgrad_lib(), "tk_lab_gru_wgrad_splits")


def test_plan_and_workspace_arithmetic(labenv):
    """The launch plan is a function of (T, N, H, I, cu_count): tiles x runs fill the CUs and never exceed them, the
    runs are whole 16-row blocks that cover the T N rows with none empty, no partial result covers more than 8192 rows,
    and the workspace is one partial result [3H][I + H] | [3H] | [H] per (run, part)."""
    labenv.lib()
    W = _lib.gru_wgrad_lib()
    assert _lib.is_lab()
    for T, N, H, I, cus in [(1, 5, 16, 7, 256), (2, 3, 16, 1, 256), (37, 5, 32, 16, 256), (25, 70, 96, 20, 256),
                            (20, 13, 192, 192, 256), (20, 130, 384, 384, 256), (20, 13, 64, 64, 256),
                            (1000, 64, 96, 96, 256), (800, 128, 192, 192, 256), (800, 128, 384, 384, 304),
                            (800, 256, 384, 384, 8), (4000, 128, 128, 16, 256), (100000, 8, 64, 300, 64)]:
        p, K = _plan(W, T, N, H, I, cus), T * N
        tiles = p["tiles_m"] * p["tiles_n"]
        assert p["tiles_m"] == -(-3 * H // 128) and p["tiles_n"] == -(-I // 128) + -(-H // 128)
        assert tiles * p["runs"] <= max(cus, tiles) and p["grid"] >= tiles * p["runs"] and p["grid"] % 8 == 0
        assert p["run_rows"] % 16 == 0 and p["part_rows"] % 16 == 0 and p["part_rows"] <= 8192
        assert (p["runs"] - 1) * p["run_rows"] < K <= p["runs"] * p["run_rows"]         # no empty run
        assert p["parts"] * p["part_rows"] >= p["run_rows"] > (p["parts"] - 1) * p["part_rows"]
        assert p["slabs"] == p["runs"] * p["parts"]
        slab = -(-(3 * H * (I + H) + 3 * H + H) // 4) * 4
        assert W.tk_gru_weight_grad_workspace_bytes(T, N, H, I, cus) == p["slabs"] * slab * 4
    # the release library plans the same (it has no hook to say otherwise)
    R = ctypes.CDLL(os.path.join(_lib.CSRC, _lib.GRU_WGRAD_LIBNAME))
    R.tk_gru_weight_grad_workspace_bytes.restype = ctypes.c_size_t
    R.tk_gru_weight_grad_workspace_bytes.argtypes = [ctypes.c_size_t] * 4 + [ctypes.c_int]
    for shape in [(800, 128, 384, 384), (1000, 64, 96, 96), (25, 70, 96, 20)]:
        assert R.tk_gru_weight_grad_workspace_bytes(*shape, CUS) == W.tk_gru_weight_grad_workspace_bytes(*shape, CUS) > 0
    # a zero size, an odd H (the seam at 2H must fall between two float4s), an output beyond 32-bit indices, no CUs
    for shape in [(0, 5, 16, 7), (3, 0, 16, 7), (3, 5, 0, 7), (3, 5, 16, 0), (3, 5, 15, 7), (3, 5, 97, 96),
                  (1 << 20, 1 << 12, 16, 16), (3, 5, 1 << 20, 1 << 20)]:
        assert W.tk_gru_weight_grad_workspace_bytes(*shape, CUS) == 0, shape
        assert _plan(W, *shape) is None
    assert W.tk_gru_weight_grad_workspace_bytes(3, 5, 16, 7, 0) == 0
    # the hook: the rows are cut into that many runs, as far as whole blocks go (260 rows are 17 blocks: 7 runs -> 6 of 3)
    try:
        got = []
        for splits in (1, 2, 3, 7):
            W.tk_lab_gru_wgrad_splits(splits)
            p = _plan(W, 20, 13, 64, 64)
            got.append((p["runs"], p["run_rows"]))
        assert got == [(1, 272), (2, 144), (3, 96), (6, 48)]
    finally:
        W.tk_lab_gru_wgrad_splits(0)


def test_bad_arguments_are_refused_before_any_launch():
    """NULL -> TK_ERR_BAD_ARG (db_hh apart: it may be NULL), a workspace one byte short or of size zero ->
    TK_ERR_WORKSPACE, T = 0 or an odd H -> TK_ERR_UNSUPPORTED: decided on the host (the pointers here are never
    dereferenced: there is no GPU in this test)."""
    W = _lib.gru_wgrad_lib()
    T, N, H, I = 37, 5, 16, 16
    need = W.tk_gru_weight_grad_workspace_bytes(T, N, H, I, CUS)
    assert need > 0
    p = [ctypes.c_void_p(4096 * (i + 1)) for i in range(9)]     # dgates, dq, x, y, dw_ih, dw_hh, db_ih, db_hh, workspace

    def call(ptrs, wsb, shape=(T, N, H, I)):
        return W.tk_gru_weight_grad_dev(*ptrs[:4], *shape, 0, CUS, *ptrs[4:9], wsb, None)

    for i in (0, 1, 2, 3, 4, 5, 6, 8):
        assert call(p[:i] + [ctypes.c_void_p(0)] + p[i + 1:], need) == BAD_ARG, i
    assert call(p[:8] + [ctypes.c_void_p(4096 + 4)], need) == BAD_ARG       # the workspace is 16-byte aligned
    assert call(p, need - 1) == WORKSPACE
    assert call(p, 0) == WORKSPACE
    assert call(p[:7] + [ctypes.c_void_p(0)] + p[8:], need - 1) == WORKSPACE    # (db_hh = NULL is not a bad argument)
    assert call(p, need, (0, N, H, I)) == UNSUPPORTED
    assert call(p, need, (T, N, 15, I)) == UNSUPPORTED


# ---------------------------------------------------------------------------------------------------------------------
# on the GPU
# ---------------------------------------------------------------------------------------------------------------------

def _reference(dg, dq, x, y, reverse, dtype=torch.float64):
    """The four results in `dtype` on the tensors' device, as plain products (float64: the reference)."""
    T, N, H = y.shape
    dg, dq, x, y = (t.to(dtype) for t in (dg, dq, x, y))
    d = dg.reshape(T * N, 3 * H)
    a = torch.cat([dg[:, :, :2 * H], dq], dim=2)
    if T > 1:
        sl, hp = (slice(0, T - 1), y[1:]) if reverse else (slice(1, T), y[:-1])
        w_hh = a[sl].reshape(-1, 3 * H).t() @ hp.reshape(-1, H)
    else:
        w_hh = torch.zeros(3 * H, H, dtype=dtype, device=dg.device)
    b_ih = d.sum(0)
    return dict(w_ih=d.t() @ x.reshape(T * N, -1), w_hh=w_hh, b_ih=b_ih,
                b_hh=torch.cat([b_ih[:2 * H], dq.reshape(T * N, H).sum(0)]))


@functools.lru_cache(maxsize=None)
def _case(T, N, H, I):
    """dG, dq (drawn independently of dG: the third slab of dW_hh read from the wrong one is a gross error), x, y
    (float32, host) with the first and the last time step at 50 x the rest -- a dropped or doubled boundary row, or a
    shift the wrong way, is then a gross error -- and the float64 results for both directions.  Computed once, shared,
    never written."""
    g = torch.Generator().manual_seed(2000 * T + 10 * N + H + I)
    dg, dq, x, y = (torch.randn(T, N, C, generator=g) for C in (3 * H, H, I, H))
    for t in (dg, dq, x, y):
        t[0] *= 50
        t[-1] *= 50
    return dg, dq, x, y, {reverse: _reference(dg, dq, x, y, reverse) for reverse in (False, True)}


def _gemms(dg, dq, x, y, reverse):
    """The lines of layers._gru_grads_from_dgates that the kernel replaces, on the device tensors."""
    T, N, H = y.shape
    w_ih = layers._time_sum_tn(dg, x)
    if T > 1:
        sl, hp = (slice(0, T - 1), y[1:]) if reverse else (slice(1, T), y[:-1])
        w_hh = torch.cat([layers._time_sum_tn(dg[sl][:, :, :2 * H], hp), layers._time_sum_tn(dq[sl], hp)])
    else:
        w_hh = torch.zeros(3 * H, H, device=dg.device)
    b_ih = dg.view(T * N, 3 * H).sum(0)
    return dict(w_ih=w_ih, w_hh=w_hh, b_ih=b_ih, b_hh=torch.cat([b_ih[:2 * H], dq.view(T * N, H).sum(0)]))


def _kernel(W, dg, dq, x, y, reverse, poison=None, want_b_hh=True):
    T, N, H = y.shape
    I = x.shape[2]
    dev = dg.device
    wsb = W.tk_gru_weight_grad_workspace_bytes(T, N, H, I, CUS)
    assert wsb > 0
    ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)
    if poison is not None:
        ws.fill_(poison)
    out = {k: torch.full(s, float("nan"), device=dev) for k, s in zip(KEYS, ((3 * H, I), (3 * H, H), (3 * H,), (3 * H,)))}
    rc = W.tk_gru_weight_grad_dev(_lib.ptr(dg), _lib.ptr(dq), _lib.ptr(x), _lib.ptr(y), T, N, H, I, int(reverse), CUS,
                                  _lib.ptr(out["w_ih"]), _lib.ptr(out["w_hh"]), _lib.ptr(out["b_ih"]),
                                  _lib.ptr(out["b_hh"] if want_b_hh else None), _lib.ptr(ws), wsb, _lib.stream_ptr())
    assert rc == OK
    torch.cuda.synchronize()
    return out


def _errors(got, ref):
    return {k: (got[k].double().cpu() - r).abs().max().item() / (r.abs().max().item() or 1.0) for k, r in ref.items()}


def _check(T, N, H, I, dev, W):
    dg, dq, x, y, ref = _case(T, N, H, I)
    dg, dq, x, y = dg.to(dev), dq.to(dev), x.to(dev), y.to(dev)
    outs = {}
    for reverse in (False, True):
        e_gemm = _errors(_gemms(dg, dq, x, y, reverse), ref[reverse])
        outs[reverse] = _kernel(W, dg, dq, x, y, reverse)
        e_hip = _errors(outs[reverse], ref[reverse])
        print("gru wgrad (T, N, H, I) = %s reverse %d: kernel %s, GEMMs %s" % ((T, N, H, I), reverse, e_hip, e_gemm))
        assert set(e_hip) == set(KEYS)
        for k in KEYS:
            assert e_hip[k] <= 2 * e_gemm[k] + 2e-6, (T, N, H, I, reverse, k, e_hip[k], e_gemm[k])
        assert torch.equal(outs[reverse]["b_hh"][:2 * H], outs[reverse]["b_ih"][:2 * H])
        if T == 1:
            assert outs[reverse]["w_hh"].abs().max().item() == 0.0
    return outs


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", [(1, 5, 16, 7), (2, 3, 16, 1), (37, 5, 32, 16), (25, 70, 96, 20),
                                     (20, 13, 192, 192), (20, 130, 384, 384), (9, 11, 96, 21)])
def test_kernel_matches_float64_as_the_gemms_do(gpu_device, T, N, H, I):
    """K smaller than one block, dW_hh exactly zero and the seam inside the first tile; one shifted pair and I = 1; a
    ragged last block; seams at 192 and 288 inside tiles with ragged I and N; the general path at a model size; the
    aligned path, several tiles each way.  The three instantiations: whole tiles (384, 384), 16-byte loads with ragged
    tiles (I and H multiples of 4) and the guarded loads (I = 7, 1 and, the seams inside tiles again, 21)."""
    _check(T, N, H, I, gpu_device, _lib.gru_wgrad_lib())


@pytest.mark.gpu
def test_forced_runs_agree_and_match_float64(gpu_device, labenv):
    """(20, 13, 64, 64) cut into 1, 2, 3 and 7 runs (realised as 1, 2, 3 and 6: test_plan_and_workspace_arithmetic):
    the boundaries, multiples of 16 rows, fall inside time steps of 13 rows and the shifted read of y crosses them."""
    labenv.lib()
    W = _lib.gru_wgrad_lib()
    T, N, H, I = 20, 13, 64, 64
    ref = _case(T, N, H, I)[4]
    dg, dq, x, y = (t.to(gpu_device) for t in _case(T, N, H, I)[:4])
    outs = []
    try:
        for splits in (1, 2, 3, 7):
            W.tk_lab_gru_wgrad_splits(splits)
            outs.append(_check(T, N, H, I, gpu_device, W))
    finally:
        W.tk_lab_gru_wgrad_splits(0)
    for reverse in (False, True):
        e_gemm = _errors(_gemms(dg, dq, x, y, reverse), ref[reverse])
        for i in range(len(outs)):
            for j in range(i):
                for k, r in ref[reverse].items():
                    diff = (outs[i][reverse][k] - outs[j][reverse][k]).abs().max().item() / r.abs().max().item()
                    assert diff <= 2 * e_gemm[k] + 2e-6, (i, j, reverse, k, diff)


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", [(20, 130, 384, 384), (25, 70, 96, 20)])
def test_two_calls_are_bit_identical(gpu_device, T, N, H, I):
    """... whatever the workspace held before either; db_hh[:2H] is db_ih[:2H]; db_hh = NULL changes nothing else."""
    W = _lib.gru_wgrad_lib()
    dg, dq, x, y = (t.to(gpu_device) for t in _case(T, N, H, I)[:4])
    for reverse in (False, True):
        a = _kernel(W, dg, dq, x, y, reverse, poison=float("nan"))
        b = _kernel(W, dg, dq, x, y, reverse, poison=1e30)
        c = _kernel(W, dg, dq, x, y, reverse, poison=float("nan"), want_b_hh=False)
        for k in KEYS:
            assert bool(torch.isfinite(a[k]).all()), (reverse, k)
            assert torch.equal(a[k], b[k]), (reverse, k)
            if k != "b_hh":
                assert torch.equal(a[k], c[k]), (reverse, k)
        assert torch.equal(a["b_hh"][:2 * H], a["b_ih"][:2 * H])
        assert bool(torch.isnan(c["b_hh"]).all())       # (left as it was)


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_zero_rows_add_exactly_zero(gpu_device, reverse):
    """Rows of dG and dq that are exactly 0 over a ragged set of (t, n) -- what training with per-column lengths hands
    the kernel, here any set -- with x large at those rows and y large at the rows they multiply (y at the previous
    step of the same column): bit-identical to the result with those rows of x and y zeroed."""
    W = _lib.gru_wgrad_lib()
    T, N, H, I = 25, 70, 96, 20
    dg, dq, x, y = (t.clone() for t in _case(T, N, H, I)[:4])
    mask = torch.rand(T, N, generator=torch.Generator().manual_seed(5)) < 0.3
    mask[3], mask[:, 7] = True, True
    assert 0 < int(mask.sum()) < T * N
    dg[mask], dq[mask] = 0.0, 0.0
    ymask = torch.zeros_like(mask)      # the row of y that row (t, n) of A multiplies, where there is one
    if reverse:
        ymask[1:] = mask[:-1]
    else:
        ymask[:-1] = mask[1:]
    # ... and that no other row of A multiplies, since (t, n) -> (t_prev, n) is one to one
    got = []
    for fill in (1e6, 0.0):
        xf, yf = x.clone(), y.clone()
        if fill:
            xf[mask] *= fill
            yf[ymask] *= fill
        else:
            xf[mask], yf[ymask] = 0.0, 0.0
        got.append(_kernel(W, *(t.to(gpu_device) for t in (dg, dq, xf, yf)), reverse))
    for k in KEYS:
        assert bool(torch.isfinite(got[0][k]).all()) and got[0][k].abs().max().item() > 0, k
        assert torch.equal(got[0][k], got[1][k]), (reverse, k)


def _rnn(layer):
    return layer.layer.rnn if isinstance(layer, layers.Reverse) else layer.rnn


def _layer_grads(layer, call, x, dy, switch):
    old = layers.USE_HIP_GRU_WGRAD
    layers.USE_HIP_GRU_WGRAD = switch
    try:
        x = x.detach().clone().requires_grad_(True)
        for p in layer.parameters():
            p.grad = None
        y = call(x)
        (y * dy).sum().backward()
    finally:
        layers.USE_HIP_GRU_WGRAD = old
    rnn = _rnn(layer)
    out = {"y": y, "x": x.grad, "w_ih": rnn.weight_ih_l0.grad, "w_hh": rnn.weight_hh_l0.grad, "b_ih": rnn.bias_ih_l0.grad,
           "b_hh": rnn.bias_hh_l0.grad}
    return {k: v.detach().clone() for k, v in out.items() if v is not None}


def _on_against_off(layer, call, x, dy, dev, live, what):
    """The layer's parameter gradients with the kernel and with the GEMMs, both against the float64 layer on the CPU."""
    ref_layer = copy.deepcopy(layer).double()
    ref = _layer_grads(ref_layer, lambda v: call(ref_layer, v), x.double(), dy.double(), True)
    layer = layer.to(dev)
    xg, dyg = x.to(dev), dy.to(dev)
    before = dict(layers.gru_wgrad_calls)
    on = _layer_grads(layer, lambda v: call(layer, v), xg, dyg, True)
    assert layers.gru_wgrad_calls == dict(before, kernel=before["kernel"] + 1), "the kernel did not run"
    off = _layer_grads(layer, lambda v: call(layer, v), xg, dyg, False)
    assert layers.gru_wgrad_calls == dict(before, kernel=before["kernel"] + 1, gemm=before["gemm"] + 1)
    # y and dx do not pass through the kernel
    assert torch.equal(on["y"], off["y"]) and torch.equal(on["x"], off["x"])
    keys = KEYS if live else KEYS[:3]
    assert set(on) == set(off) == set(ref) == {"y", "x"} | set(keys)
    for k in keys:
        scale = ref[k].abs().max().item()
        e_on = (on[k].double().cpu() - ref[k]).abs().max().item() / scale
        e_off = (off[k].double().cpu() - ref[k]).abs().max().item() / scale
        print("%s %s: kernel %.3g, GEMMs %.3g" % (what, k, e_on, e_off))
        assert e_on <= 2 * e_off + 2e-6, (what, k, e_on, e_off)


@pytest.mark.gpu
@pytest.mark.parametrize("live", [False, True], ids=["frozen_b_hh", "live_b_hh"])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T,N,H,I", [(37, 5, 32, 16), (12, 9, 256, 40)])
def test_through_the_layer_with_the_switch_on_and_off(gpu_device, T, N, H, I, reverse, live):
    torch.manual_seed(11 + T)
    gru = layers.GruMod(I, H)
    if live:
        gru.rnn.bias_hh_l0.requires_grad_(True)
        with torch.no_grad():
            gru.rnn.bias_hh_l0.normal_(0.0, 0.5)
    layer = layers.Reverse(gru) if reverse else gru
    x = torch.randn(T, N, I)
    dy = torch.randn(T, N, H) / (T * N) ** 0.5
    assert layers.hip_gru_workspace_bytes(copy.deepcopy(gru).to(gpu_device).rnn, x.to(gpu_device)) > 0
    _on_against_off(layer, lambda m, v: m(v), x, dy, gpu_device, live,
                    "layer (T, N, H, I) = %s reverse %d live %d" % ((T, N, H, I), reverse, live))


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
def test_through_the_layer_with_lengths(gpu_device, reverse, monkeypatch):
    """Training with per-column lengths reaches the same function: dG, dq and y are 0 beyond every length."""
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)
    T, N, H, I = 20, 6, 64, 16
    lens = [T, 0, 7, 13, 1, T]
    torch.manual_seed(29)
    gru = layers.GruMod(I, H)
    gru.rnn.bias_hh_l0.requires_grad_(True)
    x = torch.randn(T, N, I)
    dy = torch.randn(T, N, H) / (T * N) ** 0.5
    before = dict(layers.rnn_varlen_calls)
    _on_against_off(gru, lambda m, v: m(v, reverse=reverse, lengths=lens), x, dy, gpu_device, True,
                    "layer with lengths reverse %d" % reverse)
    assert layers.rnn_varlen_calls == dict(before, saved=before["saved"] + 2), "not the launch with lengths"


@pytest.mark.gpu
def test_captured_forward_and_backward_replay_bit_identical(gpu_device):
    """One forward and backward of a GruMod captured on one stream: two replays give the parameter gradients of the
    eager call, bit for bit (nothing is allocated or synchronised inside tk_gru_weight_grad_dev)."""
    torch.manual_seed(7)
    dev = gpu_device
    T, N, H, I = 16, 4, 64, 16
    layer = layers.GruMod(I, H).to(dev)
    layer.rnn.bias_hh_l0.requires_grad_(True)
    params = [p for p in layer.parameters() if p.requires_grad]
    assert len(params) == 4
    x = torch.randn(T, N, I, device=dev)
    dy = torch.randn(T, N, H, device=dev)

    def step():
        return torch.autograd.grad((layer(x) * dy).sum(), params)

    strict = _lib.is_strict()
    _lib.set_strict(False)
    try:
        before = dict(layers.gru_wgrad_calls)
        eager = [v.detach().clone() for v in step()]
        assert layers.gru_wgrad_calls == dict(before, kernel=before["kernel"] + 1)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = step()
        assert layers.gru_wgrad_calls == dict(before, kernel=before["kernel"] + 3)
        for _ in range(2):
            for v in out:
                v.detach().fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            for v, e in zip(out, eager):
                assert torch.equal(v.detach(), e)
        _lib.raise_if_nonfinite()
    finally:
        _lib.set_strict(strict)
