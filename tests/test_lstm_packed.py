"""The packed-FMA matvec of the LSTM recurrence at H 256, U 64, C 2 (csrc/lstm_kernels.hip: pk_fma_lo, pk_fma_hi): the two
batch columns of a group are the two halves of one v_pk_fma_f32, the weight broadcast out of a register pair of two
consecutive weights.  Each half rounds as fmaf does and no sum changes its operands or their order, so every output bit
is that of the plain FMAs.  The backward's block path takes it (lstm_bwd_kernel, and its VL form).  The forward was
written the same way, gave the same bits and measured slower, so it keeps its plain FMAs ("Packed-FMA
matvec"); its comparisons stay here, as what a packed forward has to meet and as the producer of what the backward reads.

All at H 256, N = 3 (two groups, the second ragged with one column: 8 workgroups), T = 5 and T = 1, both directions, at
the C ABI, every output between guards over a sentinel (tests/test_lstm_fwd_rows.py):

  * forward: y, gates and c of the release launch (256, 64, 2) are, as bits, those of the lab build's launch forced to 32
    units, (256, 32, 4), which shares the lanes, the weights and the tree;
  * forward with the lengths {5, 2, 0}: the saving VL form and the VL forms that save nothing give one y, and a column
    of length L is, as bits, the (256, 32, 4) launch on its first L steps alone, 0 from L on;
  * backward: dgates of (256, 64, 2), packed, are, as bits, those of the same columns through (256, 64, 4), which keeps
    plain FMAs (the lab build at 16 admitted columns; a column's bits do not depend on C, csrc/lstm_bwd_layout.h); with
    the lengths above a column of the VL form is the (256, 64, 4) launch on its first L steps alone, 0 from L on;
  * the same comparisons on a second set of values whose W_hh, gx and dy hold exact zeros, negative zeros and subnormals:
    the packed and the plain instruction must treat them alike;
  * against float64: the forward's outputs and dgates inside the allowance of tests/test_rnn_instantiations.py (2 x
    MIOpen's own error + 2e-6, `_allowed` there).

After a non-zero status word or return code this module launches nothing more."""
import ctypes
import functools

import pytest
import torch

from taiyaki_amd import _lib
from tests import test_lstm_bwd_layout as layout
from tests import test_lstm_fwd_lanes as lanes
from tests import test_lstm_fwd_rows as rows
from tests import test_rnn_instantiations as insts

pytestmark = pytest.mark.gpu

H, N = 256, 3
STEPS = [5, 1]
LENGTHS = (5, 2, 0)
_cus = rows._cus
_stopped = []


@pytest.fixture(autouse=True)
def _nothing_after_a_bad_status():
    if _stopped:
        pytest.fail("not run: an earlier launch of this module ended with %s" % (_stopped[0],))


def _finish(rc, status, what):
    if rc != 0:
        _stopped.append((what, "rc", rc))
    _lib.check(rc, what)
    torch.cuda.synchronize()
    word = int(status.item())
    if word != 0:
        _stopped.append((what, "status", word))
    assert word == 0, (what, word)


def _lens(T):
    return [min(v, T) for v in LENGTHS]


def _plan(n, dev, units=0, cols=0):
    """(U, C) of the lab build's launch at n columns with the units per workgroup and the admitted columns forced."""
    L = _lib.use_lab(True)
    try:
        L.tk_lab_lstm_units(units)
        L.tk_lab_lstm_cols(cols)
        out = (ctypes.c_size_t * 8)()
        assert L.tk_lab_lstm_geometry(n, H, _cus(dev), out)
        return int(out[2]), int(out[3])
    finally:
        L.tk_lab_lstm_units(0)
        L.tk_lab_lstm_cols(0)
        _lib.use_lab(False)


def test_the_launches_compared_are_the_instantiations_named(gpu_device):
    for n in (N, 1):
        assert _plan(n, gpu_device) == (64, 2), "release rule: the backward's packed FMAs"
        assert _plan(n, gpu_device, units=32) == (32, 4), "forward's plain reference"
        assert _plan(n, gpu_device, cols=16) == (64, 4), "backward's plain reference"


@functools.lru_cache(maxsize=None)
def _case(T, odd):
    """gx, a random dense W_hh and dy on the host.  odd: an eighth each of W_hh, gx and dy is +0, -0 and a subnormal of
    either sign."""
    g = torch.Generator().manual_seed(50000 + 10 * T + odd)
    gx = torch.randn(T, N, 4 * H, generator=g)
    whh = torch.randn(4 * H, H, generator=g) / H ** 0.5
    dy = torch.randn(T, N, H, generator=g) / (T * N) ** 0.5
    if odd:
        tiny = torch.finfo(torch.float32).tiny
        out = []
        for t in (gx, whh, dy):
            kind = torch.randint(0, 8, t.shape, generator=g)
            sub = (torch.rand(t.shape, generator=g) * 2 - 1) * tiny * 0.5
            t = torch.where(kind == 0, torch.zeros_like(t), t)
            t = torch.where(kind == 1, -torch.zeros_like(t), t)
            t = torch.where(kind == 2, sub, t)
            bits = t.view(torch.int32)
            assert int((bits == 0).sum()) > 0 and int((bits == -2 ** 31).sum()) > 0, "zeros of both signs"
            assert int(((t != 0) & (t.abs() < tiny)).sum()) > 0, "subnormals"
            out.append(t)
        gx, whh, dy = out
    return gx, whh, dy


def _bits_equal(got, want, what, names=("y", "gates", "cell")):
    for name, a, b in zip(names, got, want):
        if a is None or b is None:
            continue
        differ = int((a.view(torch.int32) != b.view(torch.int32)).sum().item())
        assert differ == 0, (what, name, "elements that differ as bits", differ, (a - b).abs().max().item())


# ---------------------------------------------------------------------------------------------------------------------
# forward
# ---------------------------------------------------------------------------------------------------------------------
def _plain_fwd(gx, whh, rev):
    """The lab build forced to 32 units, (256, 32, 4): plain FMAs."""
    return lanes._run("lab", gx, whh, None, rev, units=32)


@pytest.mark.parametrize("odd", [0, 1], ids=["random", "zeros-subnormals"])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
def test_forward_bits_are_those_of_the_plain_fmas(gpu_device, T, rev, odd):
    gx, whh, _ = (t.to(gpu_device) for t in _case(T, odd))
    _bits_equal(lanes._run("plain", gx, whh, None, rev), _plain_fwd(gx, whh, rev), ("forward", T, rev, odd))


@pytest.mark.parametrize("odd", [0, 1], ids=["random", "zeros-subnormals"])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
def test_forward_with_lengths_is_the_plain_fmas_on_each_columns_own_steps(gpu_device, T, rev, odd):
    dev = gpu_device
    gx, whh, _ = (t.to(dev) for t in _case(T, odd))
    lens = _lens(T)
    saving = lanes._run("vltrain", gx, whh, lens, rev)
    for build in ("varlen", "wide", "wide_y"):                             # varlen, wide_y: the y-only form
        _bits_equal(lanes._run(build, gx, whh, lens, rev), saving, ("forward, lengths", build, T, rev, odd))
    _bits_equal(lanes._run("vltrain", gx, whh, None, rev), lanes._run("plain", gx, whh, None, rev),
                ("forward, lengths NULL", T, rev, odd))
    for n, L in enumerate(lens):
        for name, t in zip(("y", "gates", "cell"), saving):
            assert bool((t[L:, n] == 0).all()), (name, n, "a step at or beyond the length is 0")
        if L:
            alone = _plain_fwd(gx[:L, n:n + 1].contiguous(), whh, rev)
            _bits_equal([t[:L, n:n + 1] for t in saving], alone, ("forward, lengths", "column %d" % n, T, rev, odd))


# ---------------------------------------------------------------------------------------------------------------------
# backward
# ---------------------------------------------------------------------------------------------------------------------
def _backward(build, whh, gates, cell, dy, lens, rev):
    """dgates of one build between guards over a sentinel: "plain" (tk_lstm_backward_dev, the release library:
    (256, 64, 2), packed), "c4" (the same entry of the lab library at 16 admitted columns: (256, 64, 4), plain FMAs) or
    "vltrain" (tk_lstm_backward_varlen_dev: (256, 64, 2) with lengths, packed)."""
    T, n, _ = dy.shape
    dev, cus, P = dy.device, _cus(dy.device), _lib.ptr
    flat, dg = rows._guarded((T, n, 4 * H), dev, 0)
    if build in ("plain", "c4"):
        assert lens is None
        L = _lib.use_lab(build == "c4")
        try:
            if build == "c4":
                L.tk_lab_lstm_units(0)
                L.tk_lab_lstm_cols(16)
            wsb = L.tk_lstm_workspace_bytes(n, H, cus)
            ws, status = layout._scratch(wsb, dev)
            rc = L.tk_lstm_backward_dev(P(whh), P(gates), P(cell), P(dy), T, n, H, rev, cus, P(dg), P(ws), wsb,
                                        P(status), _lib.stream_ptr())
        finally:
            if build == "c4":
                L.tk_lab_lstm_cols(0)
            _lib.use_lab(False)
    else:
        assert build == "vltrain"
        V = _lib.varlen_train_lib()
        wsb = V.tk_rnn_varlen_train_workspace_bytes(_lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"], n, H, cus)
        ws, status = layout._scratch(wsb, dev)
        rc = V.tk_lstm_backward_varlen_dev(P(whh), P(gates), P(cell), P(dy), P(layout._lens(lens, dev)), T, n, H, rev,
                                           cus, P(dg), P(ws), wsb, P(status), _lib.stream_ptr())
    _finish(rc, status, "lstm backward (%s)" % build)
    assert rows._guards_intact(flat, 0, dg.numel()), (build, "dgates: a store outside the tensor")
    unwritten = int((dg == rows.SENTINEL).sum().item())
    assert unwritten == 0, (build, "dgates: elements not stored", unwritten)
    assert bool(torch.isfinite(dg).all()), build
    return dg


@pytest.mark.parametrize("odd", [0, 1], ids=["random", "zeros-subnormals"])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
def test_backward_bits_are_those_of_the_plain_fmas(gpu_device, T, rev, odd):
    gx, whh, dy = (t.to(gpu_device) for t in _case(T, odd))
    _, gates, cell = lanes._run("plain", gx, whh, None, rev)
    gates, cell = gates.contiguous(), cell.contiguous()
    got = _backward("plain", whh, gates, cell, dy, None, rev)
    _bits_equal([got], [_backward("c4", whh, gates, cell, dy, None, rev)], ("backward", T, rev, odd), ["dgates"])
    _bits_equal([_backward("vltrain", whh, gates, cell, dy, None, rev)], [got], ("backward, lengths NULL", T, rev, odd),
                ["dgates"])


@pytest.mark.parametrize("odd", [0, 1], ids=["random", "zeros-subnormals"])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
def test_backward_with_lengths_is_the_plain_fmas_on_each_columns_own_steps(gpu_device, T, rev, odd):
    gx, whh, dy = (t.to(gpu_device) for t in _case(T, odd))
    lens = _lens(T)
    _, gates, cell = lanes._run("vltrain", gx, whh, lens, rev)
    gates, cell = gates.contiguous(), cell.contiguous()
    got = _backward("vltrain", whh, gates, cell, dy, lens, rev)
    for n, L in enumerate(lens):
        assert bool((got[L:, n] == 0).all()), (n, "dgates at or beyond the length are 0")
        if L:
            col = lambda t: t[:L, n:n + 1].contiguous()
            alone = _backward("c4", whh, col(gates), col(cell), col(dy), None, rev)
            _bits_equal([got[:L, n:n + 1]], [alone], ("backward, lengths", "column %d" % n, T, rev, odd),
                        ["dgates"])


# ---------------------------------------------------------------------------------------------------------------------
# against float64
# ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _float64(T, rev):
    """y, gates, c and dgates = d (y * dy).sum() / d gx of the float64 recurrence on the random case (computed once)."""
    gx, whh, dy = _case(T, 0)
    eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, dtype=torch.float64)
    g64 = gx.double().requires_grad_(True)
    y, gates, cell = rows._float64_lstm(g64, eye, whh.double(), zero, rev)
    (y * dy.double()).sum().backward()
    return y.detach(), gates.detach(), cell.detach(), g64.grad.detach()


def _miopen(gx, whh, dy, rev):
    """MIOpen's y and dgates: nn.LSTM(4H, H) with weight_ih = 1 and zero biases, fed gx (as insts._miopen_dgates)."""
    m = torch.nn.LSTM(4 * H, H).to(gx.device)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.eye(4 * H))
        m.weight_hh_l0.copy_(whh)
        m.bias_ih_l0.zero_()
        m.bias_hh_l0.zero_()
    xin = (torch.flip(gx, (0,)) if rev else gx).detach().clone().requires_grad_(True)
    y = m(xin)[0]
    (y * (torch.flip(dy, (0,)) if rev else dy)).sum().backward()
    flip = (lambda t: torch.flip(t, (0,))) if rev else (lambda t: t)
    return flip(y.detach()), flip(xin.grad)


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
def test_outputs_match_float64_inside_miopens_bound(gpu_device, T, rev):
    gx, whh, dy = (t.to(gpu_device) for t in _case(T, 0))
    ref = _float64(T, rev)
    y, gates, cell = lanes._run("plain", gx, whh, None, rev)
    dg = _backward("plain", whh, gates.contiguous(), cell.contiguous(), dy, None, rev)
    y_mio, dg_mio = _miopen(gx, whh, dy, rev)
    e_y, e_dg = rows._rel(y_mio, ref[0]), rows._rel(dg_mio, ref[3])
    assert ref[3].abs().max().item() > 0
    for name, a, r, e_mio in (("y", y, ref[0], e_y), ("gates", gates, ref[1], e_y), ("cell", cell, ref[2], e_y),
                              ("dgates", dg, ref[3], e_dg)):
        e = rows._rel(a, r)
        print("lstm packed T %d rev %d %s: error %.3e, MIOpen's %.3e, ratio %.3f"
              % (T, rev, name, e, e_mio, e / insts._allowed(e_mio)))
        assert e <= insts._allowed(e_mio), (T, rev, name, e, e_mio)
