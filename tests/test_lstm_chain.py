"""The step schedule of the LSTM recurrence at H 256 (csrc/lstm_kernels.hip): what a step computes that does not
depend on the hand-off stands in front of its poll.  The forward at (256, 64, 2) and every backward walk their tensors
with running pointers, one step on per step; the forward reads the step before's staging block behind the matvec's
first reads and stores it behind the first group of FMAs; the backward takes tanh(c_t) and the factors of the gate
derivatives from the loads settled at the top of the step; both test give_up once, in front of the publish.  No float
operation changed its operands, so every check that has a witness is on bits.

What is new to get wrong is where a running pointer stands in the first and the last steps, so the shapes are the
shortest: T 1 (no poll, the store behind the loop alone), T 2 (one poll, one deferred store), T 3 (the staging block's
first reuse, the first prefetch two steps on) and T 5; N 1 (a half-empty group at 2 columns per workgroup), N 3 (a
ragged last group) and N 4; both directions.  Every tensor the kernels read or write starts 4 bytes off 16-byte
alignment; every output lies over a sentinel between guard bands: each element is stored, nothing outside is.

  * forward: y, c and the gates of the (256, 64, 2) launch equal, bit for bit, those of the 32-unit kernel (the lab
    build forced to 32 units), which runs the plain body this change does not touch; and they lie within 2 x MIOpen's
    own error + 2e-6 of the float64 recurrence (the rule of tests/test_lstm_fwd_rows.py);
  * backward: dgates within 2 x MIOpen's own error + 2e-6 of the float64 recurrence's gradient (the rule of
    tests/test_rnn_instantiations.py), and a column's bits the same at 2 and at 4 columns per workgroup;
  * with lengths (the training pair of the variable-length library): T 5, lengths 1, 3 and 5; forward and backward
    against the masked float64 recurrence under the same rule, zeros at and beyond every length.

The give-up path is not run here: reaching it takes a hand-off that never comes (DESIGN.md "LSTM recurrence" argues it
from the code).  After a non-zero status word or return code this module launches nothing more."""
import functools

import pytest
import torch

from taiyaki_amd import _lib
from tests import test_lstm_bwd_layout as bwd_layout
from tests import test_lstm_fwd_lanes as lanes
from tests import test_lstm_fwd_rows as rows
from tests import test_rnn_instantiations as insts

pytestmark = pytest.mark.gpu

H = 256
INST = (256, 64, 2)
STEPS = [1, 2, 3, 5]
BATCHES = [1, 3, 4]
LENGTHS = {3: (1, 3, 5), 4: (5, 1, 3, 1)}        # T 5: the lengths 1, 3 and 5, by batch
KIND = _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"]
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


def _off16(t, dev):
    """t on the device, contiguous, its first element 4 bytes past a 16-byte boundary."""
    flat = torch.empty(t.numel() + 1, dtype=t.dtype, device=dev)
    out = flat[1:].view(t.shape)
    out.copy_(t)
    assert out.data_ptr() % 16 == 4 and out.is_contiguous()
    return out


@functools.lru_cache(maxsize=None)
def _case(N, T):
    """gx, a random dense W_hh and dy on the host (seeded by the shape)."""
    g = torch.Generator().manual_seed(62000 + 10 * N + T)
    gx = torch.randn(T, N, 4 * H, generator=g)
    whh = torch.randn(4 * H, H, generator=g) / H ** 0.5
    dy = torch.randn(T, N, H, generator=g) / (T * N) ** 0.5
    return gx, whh, dy


def _on(dev, N, T):
    return tuple(_off16(t, dev) for t in _case(N, T))


@functools.lru_cache(maxsize=None)
def _forward64(N, T, rev):
    """y, gates, c of the float64 recurrence on gx (computed once, not written to afterwards)."""
    gx, whh, _ = _case(N, T)
    eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, dtype=torch.float64)
    return rows._float64_lstm(gx.double(), eye, whh.double(), zero, rev)


@functools.lru_cache(maxsize=None)
def _masked_y64(N, T, rev):
    gx, whh, _ = _case(N, T)
    eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, dtype=torch.float64)
    return insts._masked_lstm(gx.double(), eye, whh.double(), zero, LENGTHS[N], rev)


@functools.lru_cache(maxsize=None)
def _dgates64(N, T, rev, masked):
    gx, whh, dy = _case(N, T)
    return bwd_layout._dgates64(gx, whh, dy, LENGTHS[N] if masked else None, rev)


def _miopen(gx, whh, dy, rev):
    """MIOpen's y and dgates: nn.LSTM(4H, H) with weight_ih = 1 and zero biases, fed gx."""
    m = torch.nn.LSTM(4 * H, H).to(gx.device)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.eye(4 * H))
        m.weight_hh_l0.copy_(whh)
        m.bias_ih_l0.zero_()
        m.bias_hh_l0.zero_()
    xin = (torch.flip(gx, (0,)) if rev else gx).detach().clone().requires_grad_(True)
    y = m(xin)[0]
    (y * (torch.flip(dy, (0,)) if rev else dy)).sum().backward()
    return (torch.flip(y.detach(), (0,)), torch.flip(xin.grad, (0,))) if rev else (y.detach(), xin.grad)


def _is_the_lane_layouts_launch(n, dev):
    insts._check_inst(INST, n, dev)               # the release rule: (256, 64, 2) ...
    lanes._units32(INST, n, dev)                  # ... and the lab's 32 units: (256, 32, 4), the plain body


def _backward(whh, gates, cell, dy, lens, rev):
    """tk_lstm_backward_dev (lens None) or tk_lstm_backward_varlen_dev into a sentinel-filled dgates one float off
    16-byte alignment, between guards.  Asserts the guards, every element stored and finite."""
    T, N, _ = dy.shape
    dev, cus, P = dy.device, _cus(dy.device), _lib.ptr
    flat, dg = rows._guarded((T, N, 4 * H), dev, 1)
    assert dg.data_ptr() % 16 == 4
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if lens is None:
        L = _lib.lib()
        wsb = L.tk_lstm_workspace_bytes(N, H, cus)
        assert wsb > 0
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        rc = L.tk_lstm_backward_dev(P(whh), P(gates), P(cell), P(dy), T, N, H, rev, cus, P(dg), P(ws), wsb, P(status),
                                    _lib.stream_ptr())
    else:
        V = _lib.varlen_train_lib()
        wsb = V.tk_rnn_varlen_train_workspace_bytes(KIND, N, H, cus)
        assert wsb > 0
        ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
        ln = torch.tensor(lens, dtype=torch.int32, device=dev)
        rc = V.tk_lstm_backward_varlen_dev(P(whh), P(gates), P(cell), P(dy), P(ln), T, N, H, rev, cus, P(dg), P(ws), wsb,
                                           P(status), _lib.stream_ptr())
    _finish(rc, status, "lstm backward")
    assert rows._guards_intact(flat, 1, dg.numel()), "dgates: a store outside the tensor"
    unwritten = int((dg == rows.SENTINEL).sum().item())
    assert unwritten == 0, ("dgates: elements not stored", unwritten)
    assert bool(torch.isfinite(dg).all())
    return dg


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("N", BATCHES)
def test_forward_has_the_plain_bodys_bits_inside_its_bounds(gpu_device, N, T, rev):
    dev = gpu_device
    _is_the_lane_layouts_launch(N, dev)
    gx, whh, dy = _on(dev, N, T)
    got = lanes._run("plain", gx, whh, None, rev)                # (guards, every element stored: asserted there)
    lanes._same(got, lanes._run("lab", gx, whh, None, rev, units=32), (N, T, rev))
    ref = _forward64(N, T, rev)
    e_mio = rows._rel(_miopen(gx, whh, dy, rev)[0], ref[0])
    for name, a, r in zip(("y", "gates", "cell"), got, ref):
        e = rows._rel(a, r)
        print("lstm chain fwd N %d T %d rev %d %s: error %.3e, MIOpen's y %.3e, ratio %.3f"
              % (N, T, rev, name, e, e_mio, e / insts._allowed(e_mio)))
        assert e <= insts._allowed(e_mio), (N, T, rev, name, e, e_mio)


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("N", BATCHES)
def test_backward_matches_float64_inside_its_bounds(gpu_device, N, T, rev):
    dev = gpu_device
    insts._check_inst(INST, N, dev)
    gx, whh, dy = _on(dev, N, T)
    _, gates, cell = lanes._run("plain", gx, whh, None, rev)
    dg = _backward(whh, gates, cell, dy, None, rev)
    ref = _dgates64(N, T, rev, False)
    assert ref.abs().max().item() > 0
    e, e_mio = rows._rel(dg, ref), rows._rel(_miopen(gx, whh, dy, rev)[1], ref)
    print("lstm chain bwd N %d T %d rev %d dgates: error %.3e, MIOpen's %.3e, ratio %.3f"
          % (N, T, rev, e, e_mio, e / insts._allowed(e_mio)))
    assert e <= insts._allowed(e_mio), (N, T, rev, e, e_mio)


@pytest.mark.parametrize("rev", [0, 1])
def test_backward_column_has_the_same_bits_at_2_and_at_4_columns_per_workgroup(gpu_device, rev):
    dev, T = gpu_device, 5
    n4 = lanes._batch((256, 64, 4), dev)
    gx, whh, dy = _on(dev, n4, T)
    _, gates, cell = lanes._run("plain", gx, whh, None, rev)
    wide = _backward(whh, gates, cell, dy, None, rev)
    for n2 in BATCHES:
        insts._check_inst(INST, n2, dev)
        for first in (0, 1, n4 - n2):            # both column positions of a workgroup, and the ragged last group's
            sl = slice(first, first + n2)
            part = _backward(whh, _off16(gates[:, sl], dev), _off16(cell[:, sl], dev), _off16(dy[:, sl], dev), None, rev)
            assert torch.equal(part, wide[:, sl]), (rev, n2, first, (part - wide[:, sl]).abs().max().item())


@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("N", sorted(LENGTHS))
def test_training_pair_with_lengths_matches_masked_float64(gpu_device, N, rev):
    dev, T, lens = gpu_device, 5, LENGTHS[N]
    assert set(lens) == {1, 3, 5}
    insts._check_inst(INST, N, dev)
    gx, whh, dy = _on(dev, N, T)
    y, gates, cell = lanes._run("vltrain", gx, whh, list(lens), rev)
    dg = _backward(whh, gates, cell, dy, list(lens), rev)
    beyond = (torch.arange(T)[:, None] >= torch.tensor(lens)[None, :]).to(dev)
    assert int(beyond.sum()) > 0
    for name, t in zip(("y", "gates", "cell", "dgates"), (y, gates, cell, dg)):
        assert bool((t[beyond] == 0).all()), (name, "a step at or beyond the length is 0")
    y_mio, dg_mio = _miopen(gx, whh, dy, rev)
    e, e_mio = rows._rel(y, _masked_y64(N, T, rev)), rows._rel(y_mio, _forward64(N, T, rev)[0])
    print("lstm chain lengths N %d rev %d y: error %.3e, MIOpen's %.3e, ratio %.3f" % (N, rev, e, e_mio, e / insts._allowed(e_mio)))
    assert e <= insts._allowed(e_mio), (N, rev, "y", e, e_mio)
    ref = _dgates64(N, T, rev, True)
    assert ref.abs().max().item() > 0
    e, e_mio = rows._rel(dg, ref), rows._rel(dg_mio, _dgates64(N, T, rev, False))
    print("lstm chain lengths N %d rev %d dgates: error %.3e, MIOpen's %.3e, ratio %.3f" % (N, rev, e, e_mio, e / insts._allowed(e_mio)))
    assert e <= insts._allowed(e_mio), (N, rev, "dgates", e, e_mio)
