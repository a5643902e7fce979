"""Every template instantiation of the LSTM and GRU recurrences that the release rule can launch (lstm_plan in
csrc/lstm_kernels.hip, gru_plan in csrc/gru_kernels.hip), launched at least once and compared with float64.

An instantiation is named by what the kernel is compiled for, never by N: the LSTM by (H, U, C) = (size, hidden units
per workgroup, batch columns per workgroup), the GRU by (H, C).  Every GPU test reads the CU count from the device and
takes its batch from `lstm_batch` / `gru_batch`, which restate the plans' arithmetic; the CPU tests at the top hold
those two functions, and the lists below, against the library's own dispatch (tk_lab_lstm_geometry and the workspace
queries) at 256 and at 64 CUs.

The batches.  16 admitted columns (the LSTM's (16,16,16), (32,32,8), (64,64,4), (128,64,4), (256,64,4)) need
ceil(N / 8) * H / 16 > CUs: N = 8 * (CUs // (H / 16)) + 1, one column more than 8-column groups hold.  8 admitted
columns take N = 7 C + 1.  Both leave a ragged last group of one column and at least 8 groups, and with the lengths
of the variable-length tests, lengths[n] = min(P[n % 7], T), 7 being coprime to every C, every column position of a
workgroup meets every length.

What is compared, and with which allowance: the rule of tests/test_lstm_hip.py throughout, error over the tensor's
largest entry <= 2 x MIOpen's own + 2e-6, MIOpen's error measured in the same test against the same float64 tensor.
  * saving forward at the C ABI: tests/test_lstm_fwd_rows.py's guarded, sentinel-filled launch and its comparison;
  * backward at the C ABI: dgates in a buffer of the same construction, against d(y * dy).sum() / d gx of the float64
    recurrence by autograd; MIOpen's dgates is the input gradient of an nn.LSTM(4H, H) whose weight_ih is the identity
    and whose biases are zero, fed gx;
  * variable-length forwards: the masked recurrence in float64 as include/taiyaki_amd_rnn_varlen.h words it (every
    column runs all T steps; where t >= lengths[n], h (and c) are set to 0 and y[t, n] = 0); MIOpen's y error at
    full length against the unmasked float64 layer is the allowance.

What this file found when it was written: the GRU's lengths = NULL launch at H 32 and 64 was 1 ulp off
tk_gru_forward_dev from the second step on (the saving kernel had contracted h = (1 - z) n + z h_prev into an fma, its
variable-length twin had not; csrc/gru_kernels.hip now forbids the contraction).  No LSTM instantiation was wrong.
profiles/r21_rnn_instantiations.txt keeps the per-case errors beside MIOpen's.

Every launch at the C ABI asserts return code 0 and status word 0 behind the synchronise; after a non-zero status this
module launches nothing more (the remaining tests fail at once)."""
import copy
import ctypes
import functools

import pytest
import torch

from taiyaki_amd import _lib, layers
from tests import test_gru_hip, test_lstm_fwd_rows as rows, test_lstm_hip, test_rnn_varlen as varlen

# (H, U, C) of lstm_plan's release rule: U = min(64, H), C = C_admitted * 16 / U with 8 or 16 admitted columns
LSTM_INSTS = [(16, 16, 8), (16, 16, 16), (32, 32, 4), (32, 32, 8), (64, 64, 2), (64, 64, 4), (128, 64, 2),
              (128, 64, 4), (256, 64, 2), (256, 64, 4)]
# the 16-column forms below H 256: no other test has a batch that large
LSTM_UNRUN = [(16, 16, 16), (32, 32, 8), (64, 64, 4), (128, 64, 4)]
# (H, C) of gru_plan: H <= 128 one workgroup per 1 or 2 columns, H 256 groups of 4 workgroups with 4 columns
GRU_INSTS = [(32, 1), (32, 2), (64, 1), (64, 2), (96, 1), (96, 2), (128, 1), (128, 2), (256, 4)]
STEPS = [1, 2, 7]
PATTERN = lambda T: (T, 0, 1, T - 1, 2, T, 3)          # lengths[n] = min(PATTERN(T)[n % 7], T)

_ids = lambda inst: "-".join(str(v) for v in inst)


# ---------------------------------------------------------------------------------------------------------------------
# the plans, restated
# ---------------------------------------------------------------------------------------------------------------------
def lstm_rule(n, h, cus):
    """lstm_geometry and lstm_plan: 8 admitted columns where ceil(N / 8) groups of H / 16 workgroups fit the CUs, else 16
    where those fit, else nothing; U = min(64, H); C = C_admitted * 16 / U."""
    if h not in (16, 32, 64, 128, 256) or n <= 0 or cus <= 0:
        return None
    for c16 in (8, 16):
        if -(-n // c16) * (h // 16) <= cus:
            u = min(64, h)
            return (h, u, c16 * 16 // u)
    return None


def lstm_batch(inst, cus):
    h, u, c = inst
    if c * u // 16 == 16:
        return 8 * (cus // (h // 16)) + 1       # one column more than the 8-column geometry admits
    return 7 * c + 1


def gru_rule(n, h, cus):
    """gru_plan's comment: H <= 128: C = 1 if N <= CUs, otherwise 2 (any N); H 256: C = 4 and ceil(N / 4) * 4 <= CUs."""
    if h not in (32, 64, 96, 128, 256) or n <= 0 or cus <= 0:
        return None
    if h == 256:
        return (h, 4) if -(-n // 4) * 4 <= cus else None
    return (h, 1 if n <= cus else 2)


def gru_batch(inst, cus):
    h, c = inst
    if c == 1:
        return min(cus, 9)
    if c == 2:
        return (cus | 1) + 44                   # more columns than CUs, and odd
    return 7 * c + 1


def lengths_for(n, T):
    return [min(PATTERN(T)[i % 7], T) for i in range(n)]


def _lab_lstm_inst(n, h, cus):
    """(H, U, C) of the launch at (n, h, cus) from the library's own plan (tk_lab_lstm_geometry; units not forced)."""
    L = _lib.use_lab(True)
    try:
        L.tk_lab_lstm_units(0)
        out = (ctypes.c_size_t * 8)()
        if not L.tk_lab_lstm_geometry(n, h, cus, out):
            return None
        return (h, int(out[2]), int(out[3]))
    finally:
        _lib.use_lab(False)


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the matrix is the dispatch's
# ---------------------------------------------------------------------------------------------------------------------
def test_lstm_release_rule_yields_exactly_the_ten_instantiations():
    assert sorted(set(LSTM_INSTS)) == LSTM_INSTS and len(LSTM_INSTS) == 10
    assert set(LSTM_UNRUN) == {i for i in LSTM_INSTS if i[2] * i[1] // 16 == 16 and i[0] < 256}
    L = _lib.use_lab(True)
    try:
        L.tk_lab_lstm_units(0)
        out = (ctypes.c_size_t * 8)()
        for cus in (256, 64):
            seen = set()
            for h in (16, 32, 64, 128, 256):
                for n in range(1, 16 * cus + 18):           # past the last admitted batch at H 16
                    got = (h, int(out[2]), int(out[3])) if L.tk_lab_lstm_geometry(n, h, cus, out) else None
                    assert got == lstm_rule(n, h, cus), (n, h, cus, got)
                    assert (got is not None) == (L.tk_lstm_workspace_bytes(n, h, cus) > 0), (n, h, cus)
                    if got:
                        seen.add(got)
            assert seen == set(LSTM_INSTS), (cus, sorted(seen))
    finally:
        _lib.use_lab(False)


@pytest.mark.parametrize("cus", [256, 64])
def test_lstm_batches_select_their_instantiation_ragged(cus):
    V, kind = _lib.varlen_lib(), _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"]
    for inst in LSTM_INSTS:
        h, u, c = inst
        n = lstm_batch(inst, cus)
        assert _lab_lstm_inst(n, h, cus) == inst == lstm_rule(n, h, cus), (inst, n)
        assert n % c != 0 and -(-n // c) >= 3, (inst, n)
        assert _lib.lib().tk_lstm_workspace_bytes(n, h, cus) > 0 and V.tk_rnn_varlen_workspace_bytes(kind, n, h, cus) > 0
        _every_position_meets_every_length(n, c)
    for inst in LSTM_UNRUN:             # the threshold itself: one column fewer is the 8-column sibling
        h, u, c = inst
        assert _lab_lstm_inst(lstm_batch(inst, cus) - 1, h, cus) == (h, u, c // 2), inst


@pytest.mark.parametrize("cus", [256, 64])
def test_gru_batches_select_their_instantiation_ragged(cus):
    assert sorted(set(GRU_INSTS)) == GRU_INSTS and len(GRU_INSTS) == 9
    V, kind = _lib.varlen_lib(), _lib.VARLEN_DEFINES["TK_RNN_KIND_GRU"]
    ws = _lib.lib().tk_gru_workspace_bytes
    for inst in GRU_INSTS:
        h, c = inst
        n = gru_batch(inst, cus)
        assert gru_rule(n, h, cus) == inst, (inst, n)
        assert (n % c != 0 or c == 1) and -(-n // c) >= 3, (inst, n)
        assert ws(n, h, cus) > 0 and V.tk_rnn_varlen_workspace_bytes(kind, n, h, cus) > 0, (inst, n)
        _every_position_meets_every_length(n, c)
    # admission, both libraries, on either side of the rule's thresholds
    for h in (32, 64, 96, 128, 256):
        for n in (1, cus - 3, cus, cus + 1, 2 * cus + 1, 4000):
            want = gru_rule(n, h, cus) is not None
            assert (ws(n, h, cus) > 0) == want == (V.tk_rnn_varlen_workspace_bytes(kind, n, h, cus) > 0), (n, h, cus)
    # the workspace tells C at H <= 128 apart no more than it must (16 bytes either way); at H 256 it is the plan's:
    # 2 slots x groups x G (backward) x C x H granules of 8 bytes
    n = gru_batch((256, 4), cus)
    assert ws(n, 256, cus) == 2 * -(-n // 4) * 4 * 4 * 256 * 8
    assert V.tk_rnn_varlen_workspace_bytes(kind, n, 256, cus) == 2 * -(-n // 4) * 4 * 256 * 8


def _every_position_meets_every_length(n, c):
    for T in STEPS:
        lens, distinct = lengths_for(n, T), {min(p, T) for p in PATTERN(T)}
        assert all(0 <= v <= T for v in lens)
        for pos in range(c):
            assert {lens[i] for i in range(pos, n, c)} == distinct, (n, c, T, pos)


# ---------------------------------------------------------------------------------------------------------------------
# float64: the masked recurrences, written from the header's rule
# ---------------------------------------------------------------------------------------------------------------------
def _masked_lstm(x, w_ih, w_hh, b, lengths, reverse):
    """y (T, N, H) of one nn.LSTM layer, h0 = c0 = 0: every column runs all T steps; where t >= lengths[n], h and c are
    set to 0 and y[t, n] = 0."""
    T, N, _ = x.shape
    H = w_hh.shape[1]
    lens = torch.as_tensor(lengths)
    h, c, y = x.new_zeros(N, H), x.new_zeros(N, H), x.new_zeros(T, N, H)
    for s in range(T):
        t = T - 1 - s if reverse else s
        a = x[t] @ w_ih.t() + h @ w_hh.t() + b
        i, f, o = torch.sigmoid(a[:, :H]), torch.sigmoid(a[:, H:2 * H]), torch.sigmoid(a[:, 3 * H:])
        g = torch.tanh(a[:, 2 * H:3 * H])
        c = f * c + i * g
        h = o * torch.tanh(c)
        beyond = t >= lens
        h[beyond], c[beyond] = 0.0, 0.0
        y[t] = h
    return y


def _masked_gru(x, w_ih, w_hh, b_ih, b_hh, lengths, reverse):
    """y (T, N, H) of one nn.GRU layer (gates r, z, n), h0 = 0, masked as above.  lengths None: no mask."""
    T, N, _ = x.shape
    H = w_hh.shape[1]
    lens = torch.full((N,), T) if lengths is None else torch.as_tensor(lengths)
    h, y = x.new_zeros(N, H), x.new_zeros(T, N, H)
    for s in range(T):
        t = T - 1 - s if reverse else s
        gi, gh = x[t] @ w_ih.t() + b_ih, h @ w_hh.t() + b_hh
        r = torch.sigmoid(gi[:, :H] + gh[:, :H])
        z = torch.sigmoid(gi[:, H:2 * H] + gh[:, H:2 * H])
        n = torch.tanh(gi[:, 2 * H:] + r * gh[:, 2 * H:])
        h = (1.0 - z) * n + z * h
        h[t >= lens] = 0.0
        y[t] = h
    return y


def _gru_layer(H):
    """layers.GruMod at its own initialisation, with a bias_hh that is not zero."""
    gru = layers.GruMod(H, H)
    with torch.no_grad():
        gru.rnn.bias_hh_l0.normal_(0.0, 0.5)
    return gru


def _params64(rnn):
    return [p.detach().double() for p in (rnn.weight_ih_l0, rnn.weight_hh_l0, rnn.bias_ih_l0, rnn.bias_hh_l0)]


@pytest.mark.parametrize("kind", ["lstm", "gru"])
def test_masked_reference_rows_are_the_column_run_alone(kind):
    """The reference of the variable-length tests, before it judges a kernel: rows [0, len) of a column are the
    unmasked float64 recurrence (tests/test_lstm_fwd_rows.py's for the LSTM) on that column alone over len steps, in
    both directions; rows beyond are 0.  Both sides are float64 and differ by the order of a matrix product's sums."""
    H, N, T = 32, 9, 7
    torch.manual_seed(11)
    rnn = layers.Lstm(H, H).rnn if kind == "lstm" else _gru_layer(H).rnn
    w_ih, w_hh, b_ih, b_hh = _params64(rnn)
    x, lens = torch.randn(T, N, H).double(), lengths_for(N, T)
    assert set(lens) == {0, 1, 2, 3, 6, 7}
    for rev in (0, 1):
        if kind == "lstm":
            y = _masked_lstm(x, w_ih, w_hh, b_ih + b_hh, lens, rev)
            alone = lambda xs: rows._float64_lstm(xs, w_ih, w_hh, b_ih + b_hh, rev)[0]
        else:
            y = _masked_gru(x, w_ih, w_hh, b_ih, b_hh, lens, rev)
            alone = lambda xs: _masked_gru(xs, w_ih, w_hh, b_ih, b_hh, None, rev)
        for n in range(N):
            ln = lens[n]
            assert torch.equal(y[ln:, n], torch.zeros(T - ln, H).double()), (kind, rev, n)
            if ln:
                want = alone(x[:ln, n:n + 1].contiguous())[:, 0]
                assert want.abs().max().item() > 1e-3
                assert (y[:ln, n] - want).abs().max().item() <= 1e-13, (kind, rev, n)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_cus = rows._cus
_stopped = []           # the first non-zero status word or return code of this module's own launches


@pytest.fixture(autouse=True)
def _nothing_after_a_bad_status():
    if _stopped:
        pytest.fail("not run: an earlier launch of this module ended with %s" % (_stopped[0],))


def _finish(rc, status, what):
    """Return code 0, and the status word 0 behind the synchronise."""
    if rc != 0:
        _stopped.append((what, "rc", rc))
    _lib.check(rc, what)
    torch.cuda.synchronize()
    word = int(status.item())
    if word != 0:
        _stopped.append((what, "status", word))
    assert word == 0, (what, word)


def _check_inst(inst, n, dev):
    assert _lab_lstm_inst(n, inst[0], _cus(dev)) == inst, (inst, n, _cus(dev))


def _allowed(e_mio):
    return 2 * e_mio + 2e-6


# --- 2. LSTM saving forward and backward ----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("inst", LSTM_UNRUN, ids=_ids)
def test_lstm_layer_matches_float64(gpu_device, inst, reverse):
    """layers.Lstm forward and backward (y, dx, dW_ih, dW_hh, db) through tests/test_lstm_hip.py's comparison."""
    n = lstm_batch(inst, _cus(gpu_device))
    _check_inst(inst, n, gpu_device)
    test_lstm_hip._compare(5, n, inst[0], 7, reverse, gpu_device, seed=inst[2])


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", LSTM_UNRUN, ids=_ids)
def test_lstm_saved_tensors_match_float64_inside_their_bounds(gpu_device, inst, T, rev):
    H, n = inst[0], lstm_batch(inst, _cus(gpu_device))
    _check_inst(inst, n, gpu_device)
    rnn, x, ref, gx, w_hh = rows._inputs(H, n, T, gpu_device)
    got = rows._forward(gx, w_hh, rev)
    e_mio = rows._rel(rows._miopen_y(rnn, x, rev, gpu_device), ref[rev][0])
    for name, a, r in zip(("y", "gates", "cell"), got, ref[rev]):
        e = rows._rel(a, r)
        print("lstm fwd %s N %d T %d rev %d %s: error %.3e, MIOpen's y %.3e, ratio %.3f"
              % (_ids(inst), n, T, rev, name, e, e_mio, e / _allowed(e_mio)))
        assert e <= _allowed(e_mio), (inst, n, T, rev, name, e, e_mio)


def _bwd_batch(inst, dev):
    """The smallest N of tests/test_lstm_fwd_rows.py's shapes that selects the instantiation on this device, else the
    batch of `lstm_batch`."""
    cus = _cus(dev)
    known = sorted(n for h, n in rows.SHAPES if lstm_rule(n, h, cus) == inst)
    n = known[0] if known else lstm_batch(inst, cus)
    _check_inst(inst, n, dev)
    return n


def _backward(w_hh, gates, cell, dy, rev):
    """tk_lstm_backward_dev into a guarded, sentinel-filled dgates; asserts the bounds, returns dgates."""
    T, N, H = dy.shape
    dev, L = dy.device, _lib.lib()
    wsb = L.tk_lstm_workspace_bytes(N, H, _cus(dev))
    assert wsb > 0
    flat, dg = rows._guarded((T, N, 4 * H), dev, 0)
    ws, status = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.tk_lstm_backward_dev(_lib.ptr(w_hh), _lib.ptr(gates), _lib.ptr(cell), _lib.ptr(dy), T, N, H, rev,
                                _cus(dev), _lib.ptr(dg), _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr())
    _finish(rc, status, "tk_lstm_backward_dev")
    assert rows._guards_intact(flat, 0, dg.numel()), "dgates: a store outside the tensor"
    unwritten = int((dg == rows.SENTINEL).sum().item())
    assert unwritten == 0, ("dgates: elements not stored", unwritten)
    assert bool(torch.isfinite(dg).all())
    return dg


@functools.lru_cache(maxsize=None)
def _dy(H, N, T):
    g = torch.Generator().manual_seed(7000 * H + 10 * N + T)
    return torch.randn(T, N, H, generator=g) / (T * N) ** 0.5


_DGATES64 = {}


def _dgates64(H, N, T, gx, w_hh):
    """d (y * dy).sum() / d gx of the float64 recurrence on the kernel's own gx, both directions (computed once)."""
    key = (H, N, T)
    if key not in _DGATES64:
        eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, dtype=torch.float64)
        out = {}
        for rev in (0, 1):
            g64 = gx.detach().cpu().double().requires_grad_(True)
            y = rows._float64_lstm(g64, eye, w_hh.detach().cpu().double(), zero, rev)[0]
            (y * _dy(H, N, T).double()).sum().backward()
            out[rev] = g64.grad.detach()
        _DGATES64[key] = out
    return _DGATES64[key]


def _miopen_dgates(gx, w_hh, dy, rev):
    """MIOpen's dgates: the input gradient of nn.LSTM(4H, H) with weight_ih = 1 and zero biases, fed gx."""
    H = w_hh.shape[1]
    m = torch.nn.LSTM(4 * H, H).to(gx.device)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.eye(4 * H))
        m.weight_hh_l0.copy_(w_hh)
        m.bias_ih_l0.zero_()
        m.bias_hh_l0.zero_()
    xin = (torch.flip(gx, (0,)) if rev else gx).detach().clone().requires_grad_(True)
    (m(xin)[0] * (torch.flip(dy, (0,)) if rev else dy)).sum().backward()
    return torch.flip(xin.grad, (0,)) if rev else xin.grad


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", LSTM_INSTS, ids=_ids)
def test_lstm_backward_dgates_match_float64_inside_their_bounds(gpu_device, inst, T, rev):
    H, n = inst[0], _bwd_batch(inst, gpu_device)
    _, _, _, gx, w_hh = rows._inputs(H, n, T, gpu_device)
    _, gates, cell = rows._forward(gx, w_hh, rev)
    dy = _dy(H, n, T).to(gpu_device)
    dg = _backward(w_hh, gates, cell, dy, rev)
    ref = _dgates64(H, n, T, gx, w_hh)[rev]
    assert ref.abs().max().item() > 0
    e, e_mio = rows._rel(dg, ref), rows._rel(_miopen_dgates(gx, w_hh, dy, rev), ref)
    print("lstm bwd %s N %d T %d rev %d dgates: error %.3e, MIOpen's %.3e, ratio %.3f"
          % (_ids(inst), n, T, rev, e, e_mio, e / _allowed(e_mio)))
    assert e <= _allowed(e_mio), (inst, n, T, rev, e, e_mio)


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", [(16, 16, 16), (32, 32, 8), (128, 64, 4)], ids=_ids)
def test_lstm_backward_two_calls_give_the_same_bits(gpu_device, inst, rev):
    """One shape per U (16, 32, 64): the reduce-scatter sums its producers in a fixed order."""
    H, T, n = inst[0], 7, _bwd_batch(inst, gpu_device)
    _, _, _, gx, w_hh = rows._inputs(H, n, T, gpu_device)
    _, gates, cell = rows._forward(gx, w_hh, rev)
    dy = _dy(H, n, T).to(gpu_device)
    assert torch.equal(_backward(w_hh, gates, cell, dy, rev), _backward(w_hh, gates, cell, dy, rev))


# --- 3. variable-length forwards ------------------------------------------------------------------------------------
def _vl(kind, gx, whh, bhh, lens, rev):
    """tk_lstm_forward_varlen_dev / tk_gru_forward_varlen_dev into a guarded, sentinel-filled y (lens: a device int32
    tensor or None); asserts the bounds, every element stored and finite."""
    T, N, HG = gx.shape
    lstm = kind == "lstm"
    H, dev, V = HG // (4 if lstm else 3), gx.device, _lib.varlen_lib()
    wsb = V.tk_rnn_varlen_workspace_bytes(_lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM" if lstm else "TK_RNN_KIND_GRU"], N, H,
                                          _cus(dev))
    assert wsb > 0
    flat, y = rows._guarded((T, N, H), dev, 0)
    ws, status = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    tail = (T, N, H, rev, _cus(dev), _lib.ptr(y), _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr())
    if lstm:
        rc = V.tk_lstm_forward_varlen_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(lens), *tail)
    else:
        rc = V.tk_gru_forward_varlen_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(bhh), _lib.ptr(lens), *tail)
    _finish(rc, status, "tk_%s_forward_varlen_dev" % kind)
    assert rows._guards_intact(flat, 0, y.numel()), "y: a store outside the tensor"
    unwritten = int((y == rows.SENTINEL).sum().item())
    assert unwritten == 0, ("y: elements not stored (every row of y is written)", unwritten)
    assert bool(torch.isfinite(y).all())
    return y


def _check_varlen(kind, what, gx, whh, bhh, lens_host, rev, masked64, e_mio, saving):
    """The assertions of one variable-length launch and of its three siblings."""
    T, N, _ = gx.shape
    dev = gx.device
    distinct = {min(p, T) for p in PATTERN(T)}
    assert set(lens_host) == distinct, (what, sorted(set(lens_host)))
    lens = torch.tensor(lens_host, dtype=torch.int32, device=dev)
    y = _vl(kind, gx, whh, bhh, lens, rev)
    beyond = torch.arange(T, device=dev)[:, None] >= lens[None, :]                     # (T, N)
    assert int(beyond.sum().item()) > 0 or T == 0
    assert bool((y[beyond] == 0).all()), (what, "rows at and beyond the length are not exactly 0")
    e = rows._rel(y, masked64)
    print("%s: error %.3e, MIOpen's y %.3e, ratio %.3f" % (what, e, e_mio, e / _allowed(e_mio)))
    assert e <= _allowed(e_mio), (what, e, e_mio)
    # gx beyond the length is never used, whatever it holds
    poisoned = gx.clone()
    poisoned[beyond] = float("nan")
    assert bool(torch.isnan(poisoned).any())
    assert torch.equal(_vl(kind, poisoned, whh, bhh, lens, rev), y), (what, "gx beyond the length was used")
    # lengths = NULL and lengths = [T] * N: the existing forward on the whole batch, bit for bit
    want = saving()
    assert torch.equal(_vl(kind, gx, whh, bhh, None, rev), want), (what, "lengths = NULL")
    full = torch.full((N,), T, dtype=torch.int32, device=dev)
    assert torch.equal(_vl(kind, gx, whh, bhh, full, rev), want), (what, "lengths = [T] * N")


@functools.lru_cache(maxsize=None)
def _lstm_masked64(H, N, T):
    rnn, x, _ = rows._case(H, N, T)
    w_ih, w_hh, b_ih, b_hh = _params64(rnn)
    return {rev: _masked_lstm(x.double(), w_ih, w_hh, b_ih + b_hh, lengths_for(N, T), rev) for rev in (0, 1)}


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", LSTM_INSTS, ids=_ids)
def test_lstm_varlen_matches_masked_float64(gpu_device, inst, T, rev):
    H, n = inst[0], lstm_batch(inst, _cus(gpu_device))
    _check_inst(inst, n, gpu_device)
    rnn, x, ref, gx, w_hh = rows._inputs(H, n, T, gpu_device)
    e_mio = rows._rel(rows._miopen_y(rnn, x, rev, gpu_device), ref[rev][0])
    _check_varlen("lstm", "lstm VL %s N %d T %d rev %d" % (_ids(inst), n, T, rev), gx, w_hh, None,
                  lengths_for(n, T), rev, _lstm_masked64(H, n, T)[rev], e_mio,
                  lambda: varlen._lstm_saving(gx, w_hh, rev))


@functools.lru_cache(maxsize=None)
def _gru_case(H, N, T):
    """One GruMod at its own initialisation with a non-zero bias_hh, its input, and per direction the unmasked and the
    masked float64 y (computed once)."""
    torch.manual_seed(3000 * H + 10 * N + T)
    gru = _gru_layer(H)
    x = torch.randn(T, N, H)
    p = _params64(gru.rnn)
    ref = {rev: (_masked_gru(x.double(), *p, None, rev), _masked_gru(x.double(), *p, lengths_for(N, T), rev))
           for rev in (0, 1)}
    return gru, x, ref


def _miopen_gru_y(gru, x, rev, dev):
    m = copy.deepcopy(gru).to(dev)
    old = layers.USE_HIP_GRU
    try:
        layers.USE_HIP_GRU = False
        with torch.no_grad():
            assert layers.hip_gru_workspace_bytes(m.rnn, x.to(dev)) == 0
            return m(x.to(dev), reverse=bool(rev))
    finally:
        layers.USE_HIP_GRU = old


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", GRU_INSTS, ids=_ids)
def test_gru_varlen_matches_masked_float64(gpu_device, inst, T, rev):
    H, cus = inst[0], _cus(gpu_device)
    n = gru_batch(inst, cus)
    assert gru_rule(n, H, cus) == inst, (inst, n, cus)
    gru, x, ref = _gru_case(H, n, T)
    rnn = gru.rnn
    w_ih, w_hh = rnn.weight_ih_l0.detach().to(gpu_device), rnn.weight_hh_l0.detach().to(gpu_device).contiguous()
    b_hh = rnn.bias_hh_l0.detach().to(gpu_device).contiguous()
    assert float(b_hh.abs().min()) > 0
    gx = (x.to(gpu_device) @ w_ih.t() + rnn.bias_ih_l0.detach().to(gpu_device)).contiguous()
    e_mio = rows._rel(_miopen_gru_y(gru, x, rev, gpu_device), ref[rev][0])
    _check_varlen("gru", "gru VL %s N %d T %d rev %d" % (_ids(inst), n, T, rev), gx, w_hh, b_hh, lengths_for(n, T),
                  rev, ref[rev][1], e_mio, lambda: varlen._gru_saving(gx, w_hh, b_hh, rev))


# --- 4. GRU at 2 columns per workgroup ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("H", [32, 64, 128])
def test_gru_batch_larger_than_the_cu_count_matches_float64(gpu_device, H, reverse):
    """tests/test_gru_hip.py::test_batch_larger_than_the_cu_count_matches_float64 (H 96) at the other sizes of one
    workgroup per group: forward and backward through the layer."""
    cus = _cus(gpu_device)
    assert gru_rule(cus + 45, H, cus) == (H, 2)
    test_gru_hip._compare(9, cus + 45, H, 8, reverse, gpu_device, seed=6)
