"""The GruMod recurrence at hidden sizes 192 and 384 (csrc/gru_kernels.hip): the sizes that are no power of two.

The rule under test (gru_plan).  A workgroup owns U = 48 hidden units, a group is G = H / 48 workgroups that share C batch
columns and hand h (forward) and W_hh^T dG (backward) to each other, so the grid must fit one workgroup per CU.  C = 4
where ceil(N / 4) * G <= CUs; else C = 8 where ceil(N / 8) * G <= CUs; else the batch is refused.  On 256 CUs: H = 384
takes N <= 128 at 4 columns and N <= 256 at 8, H = 192 N <= 256 and N <= 512.  The workspace is the backward's granules,
2 slots x groups x G producers x C x H x 8 bytes; the forward-only library's is 2 x groups x C x H x 8.

An instantiation is named (H, C), as tests/test_rnn_instantiations.py names the GRU's, whose helpers, references and
allowance this file imports: error over the tensor's largest entry <= 2 x MIOpen's own + 2e-6, both against float64.
MIOpen saves no gates and no q in a form that can be read, and has no dq: the saved tensors take the allowance of MIOpen's
y (they are the same step's values, one activation before y), dq that of MIOpen's dgates (dq = dn_pre r, the third slab
of dgates times an activation).  The float64 recurrence with gates, q and dq is `_gru64` below; a CPU test holds it
against tests/test_rnn_instantiations.py's `_masked_gru` before it judges a kernel.

The batches: 7 * 4 + 1 = 29 columns for the 4-column forms (8 groups, the last ragged); for the 8-column forms one column
more than 4 columns admit on the device, 4 * (CUs // G) + 1 (129 at H = 384, 257 at H = 192 on 256 CUs).

Every launch at the C ABI asserts return code 0 and status word 0 behind the synchronise; after a non-zero status of this
file's launches nothing more is launched (the remaining tests fail at once)."""
import functools

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, layers
from tests import test_gru_hip, test_lstm_fwd_rows as rows, test_lstm_sizes as lstm_sizes, test_rnn_entry_checks as entry
from tests import test_rnn_instantiations as insts, test_rnn_varlen as varlen, test_rnn_varlen_train as vtrain

SIZES = (192, 384)
COLUMNS = (4, 8)
NEW_INSTS = [(192, 4), (192, 8), (384, 4), (384, 8)]
STEPS = insts.STEPS
_ids = insts._ids
_cus = rows._cus
_allowed = insts._allowed
KIND = _lib.VARLEN_DEFINES["TK_RNN_KIND_GRU"]


# ---------------------------------------------------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------------------------------------------------
def sizes_rule(n, h, cus):
    if h not in SIZES or n <= 0 or cus <= 0:
        return None
    for c in COLUMNS:
        if -(-n // c) * (h // 48) <= cus:
            return (h, c)
    return None


def last_admitted(h, cus, c=COLUMNS[-1]):
    return c * (cus // (h // 48))


def sizes_batch(inst, cus):
    h, c = inst
    return 7 * c + 1 if c == COLUMNS[0] else last_admitted(h, cus, COLUMNS[0]) + 1


def train_bytes(n, h, c):
    return 2 * -(-n // c) * (h // 48) * c * h * 8


def forward_bytes(n, h, c):
    return 2 * -(-n // c) * c * h * 8


def columns_from_bytes(n, h, nbytes):
    """C of the launch, told from the training workspace: at a ragged N (n % 8 not in {0, 5, 6, 7}) the two column counts
    round N up to different totals."""
    got = [c for c in COLUMNS if train_bytes(n, h, c) == nbytes]
    return got[0] if len(got) == 1 else None


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_workspace_query_admits_the_two_sizes_and_refuses_the_rest():
    ws = _lib.lib().tk_gru_workspace_bytes
    assert ws(128, 384, 256) == 2 * 32 * 8 * 4 * 384 * 8         # 32 groups of 8 workgroups, 4 columns: the 256 CUs
    assert ws(129, 384, 256) == 2 * 17 * 8 * 8 * 384 * 8         # 8 columns
    assert ws(256, 384, 256) > 0 and ws(257, 384, 256) == 0
    assert ws(256, 192, 256) == 2 * 64 * 4 * 4 * 192 * 8         # 64 groups of 4 workgroups, 4 columns
    assert ws(257, 192, 256) == 2 * 33 * 4 * 8 * 192 * 8         # 8 columns
    assert ws(512, 192, 256) > 0 and ws(513, 192, 256) == 0
    for h in SIZES:
        G = h // 48
        assert ws(1, h, G) > 0 and ws(1, h, G - 1) == 0
        assert ws(0, h, 256) == 0 and ws(128, h, 0) == 0 and ws(128, h, -1) == 0
    assert (last_admitted(384, 256), last_admitted(192, 256)) == (256, 512)
    for h in (16, 48, 80, 144, 240, 288, 512, 576, 768):
        assert ws(128, h, 256) == 0 and ws(1, h, 256) == 0, h


def test_rule_is_the_librarys_plan_for_every_batch():
    V, T = _lib.varlen_lib(), _lib.varlen_train_lib()
    ws = _lib.lib().tk_gru_workspace_bytes
    seen, told = set(), 0
    for cus in (256, 64):
        for h in SIZES:
            for n in range(1, last_admitted(h, cus) + 2):
                want = sizes_rule(n, h, cus)
                assert (want is None) == (n > last_admitted(h, cus)), (n, h, cus)
                q, qv, qt = ws(n, h, cus), V.tk_rnn_varlen_workspace_bytes(KIND, n, h, cus), \
                    T.tk_rnn_varlen_train_workspace_bytes(KIND, n, h, cus)
                # the three libraries admit exactly the same (N, H, CUs)
                assert (q > 0) == (qv > 0) == (qt > 0) == (want is not None), (n, h, cus)
                if want is None:
                    continue
                c = want[1]
                assert -(-n // c) * (h // 48) <= cus, "one workgroup per CU: the members of a group wait on each other"
                assert q == qt == train_bytes(n, h, c), (n, h, cus, q, qt)
                assert qv == forward_bytes(n, h, c), (n, h, cus, qv)
                if n % 8 in (1, 2, 3, 4):
                    assert columns_from_bytes(n, h, q) == c, (n, h, cus)
                    told += 1
                seen.add(want)
    assert seen == set(NEW_INSTS) and told == (512 + 256 + 128 + 64) // 2
    # the lab's forced columns are those of one workgroup per group (H <= 128): they do not apply
    L = _lib.use_lab(True)
    try:
        for cols in (1, 2):
            L.tk_lab_gru_cols(cols)
            assert L.tk_gru_workspace_bytes(29, 384, 256) == train_bytes(29, 384, 4)
            assert L.tk_gru_workspace_bytes(257, 192, 256) == train_bytes(257, 192, 8)
    finally:
        L.tk_lab_gru_cols(0)
        _lib.use_lab(False)


@pytest.mark.parametrize("cus", [256, 64])
def test_batches_select_their_instantiation_ragged(cus):
    ws = _lib.lib().tk_gru_workspace_bytes
    for inst in NEW_INSTS:
        h, c = inst
        n = sizes_batch(inst, cus)
        assert sizes_rule(n, h, cus) == inst and ws(n, h, cus) == train_bytes(n, h, c), (inst, n)
        assert c == 4 or columns_from_bytes(n, h, ws(n, h, cus)) == c, (inst, n)       # (29 columns are 32 either way)
        assert n % c != 0 and -(-n // c) >= 3, (inst, n)
        assert n >= 7 * c or cus < 256
        if n >= 7 * c:                  # (a device of 64 CUs admits 33 columns at H = 384: 5 per position at most)
            insts._every_position_meets_every_length(n, c)
    assert sizes_rule(sizes_batch((192, 8), cus) - 1, 192, cus) == (192, 4)
    assert sizes_rule(sizes_batch((384, 8), cus) - 1, 384, cus) == (384, 4)
    assert [sizes_batch(i, 256) for i in NEW_INSTS] == [29, 257, 29, 129]


GRU_ENTRIES = [name for name, v in entry.ENTRIES.items() if v[1] == "gru"]


@pytest.mark.parametrize("shape", [(5, 192, 256), (257, 192, 256), (5, 384, 256), (129, 384, 256)], ids=_ids)
@pytest.mark.parametrize("name", GRU_ENTRIES)
def test_entries_check_their_arguments_at_the_new_sizes(name, shape):
    """tests/test_rnn_entry_checks.py's calls (fake pointers that are never dereferenced: every answer comes before any
    HIP call): a short workspace, NULL pointers, and the first batch that is refused, in all three libraries."""
    assert len(GRU_ENTRIES) == 5
    e = entry.Entry(name, shape)
    c = sizes_rule(*shape)[1]
    assert e.need == (train_bytes if "backward" in name else forward_bytes)(shape[0], shape[1], c)
    assert 0 < e.need <= e.query and e.need % 16 == 0
    assert e() == entry.WORKSPACE
    assert e(workspace_bytes=e.need - 1) == entry.WORKSPACE
    assert e(nblk=0, workspace_bytes=e.need - 1) == entry.WORKSPACE
    assert e(nblk=0, workspace_bytes=e.need) == entry.OK
    for p in e.pointers:
        if p not in e.optional:
            assert e(**{p: None}) == entry.BAD_ARG, p
    assert (last_admitted(384, 256), last_admitted(192, 256)) == (256, 512)
    assert e(nbatch=last_admitted(shape[1], shape[2]) + 1) == entry.UNSUPPORTED     # the plan is asked before the workspace
    assert e(nblk=0, nbatch=last_admitted(shape[1], shape[2]) + 1, workspace_bytes=1 << 40) == entry.UNSUPPORTED


def _gru64(gx, w_hh, b_hh, lengths, reverse, eps=None):
    """One nn.GRU layer (gates r, z, n; h0 = 0) in float64 on pre-activations gx = x W_ih^T + b_ih, masked as
    include/taiyaki_amd_rnn_varlen.h words it (lengths None: no mask) -> y (T, N, H), the activations r, z, n as gates
    (T, N, 3H) and q = W_hn h + b_hn (T, N, H); the saved tensors are 0 at and beyond a length.  eps (T, N, H) is added
    to q: d / d eps is the kernel's dq."""
    T, N, _ = gx.shape
    H = w_hh.shape[1]
    lens = torch.full((N,), T) if lengths is None else torch.as_tensor(lengths)
    h = gx.new_zeros(N, H)
    ys, gs, qs = [], [], []
    for s in range(T):
        t = T - 1 - s if reverse else s
        gh = h @ w_hh.t() + b_hh
        r = torch.sigmoid(gx[t][:, :H] + gh[:, :H])
        z = torch.sigmoid(gx[t][:, H:2 * H] + gh[:, H:2 * H])
        q = gh[:, 2 * H:] if eps is None else gh[:, 2 * H:] + eps[t]
        n = torch.tanh(gx[t][:, 2 * H:] + r * q)
        keep = (t < lens).to(gx.dtype)[:, None]
        h = ((1.0 - z) * n + z * h) * keep
        ys.append(h)
        gs.append(torch.cat([r, z, n], 1) * keep)
        qs.append(q * keep)
    if reverse:
        ys, gs, qs = ys[::-1], gs[::-1], qs[::-1]
    return torch.stack(ys), torch.stack(gs), torch.stack(qs)


def _pair64(gx64, w_hh64, b_hh64, dy64, lens, rev):
    """y, gates, q, and d (y * dy).sum() / d (gx, q) of the (masked) float64 recurrence on pre-activations gx."""
    g = gx64.detach().clone().requires_grad_(True)
    eps = torch.zeros(dy64.shape, dtype=torch.float64, requires_grad=True)
    y, gates, q = _gru64(g, w_hh64, b_hh64, lens, rev, eps)
    (y * dy64).sum().backward()
    return {"y": y.detach(), "gates": gates.detach(), "c": q.detach(), "dgates": g.grad.detach(),
            "dq": eps.grad.detach()}


def test_float64_reference_is_the_projects_and_is_differentiable():
    """`_gru64` before it judges a kernel: its y is tests/test_rnn_instantiations.py's `_masked_gru` (masked and not),
    and its gradient is, column by column, that of the column run alone over its own length through `_masked_gru` by
    autograd (dq: by a central difference of q's bias), and exactly 0 at and beyond a length."""
    H, N, T = 8, 9, 7
    g = torch.Generator().manual_seed(5)
    gx, w_hh = torch.randn(T, N, 3 * H, generator=g).double(), torch.randn(3 * H, H, generator=g).double() / H ** 0.5
    b_hh, dy = 0.3 * torch.randn(3 * H, generator=g).double(), torch.randn(T, N, H, generator=g).double()
    eye, zero, lens = torch.eye(3 * H, dtype=torch.float64), torch.zeros(3 * H, dtype=torch.float64), insts.lengths_for(N, T)
    for rev in (0, 1):
        for ln in (None, lens):
            assert (_gru64(gx, w_hh, b_hh, ln, rev)[0] - insts._masked_gru(gx, eye, w_hh, zero, b_hh, ln, rev)).abs().max() \
                <= 1e-13
        got = _pair64(gx, w_hh, b_hh, dy, lens, rev)
        for n in range(N):
            ln = lens[n]
            for k, v in got.items():
                assert not v[ln:, n].any(), (k, n)
            if ln == 0:
                continue
            a = gx[:ln, n:n + 1].clone().requires_grad_(True)
            (insts._masked_gru(a, eye, w_hh, zero, b_hh, None, rev) * dy[:ln, n:n + 1]).sum().backward()
            assert (a.grad[:, 0] - got["dgates"][:ln, n]).abs().max().item() <= 1e-13
            # sum over t of dq[t] = d / d b_hn
            f = lambda b: (insts._masked_gru(gx[:ln, n:n + 1], eye, w_hh, zero, b, None, rev) * dy[:ln, n:n + 1]).sum().item()
            for j in (0, H - 1):
                d = torch.zeros(3 * H, dtype=torch.float64)
                d[2 * H + j] = 1e-6
                assert abs((f(b_hh + d) - f(b_hh - d)) / 2e-6 - got["dq"][:ln, n, j].sum().item()) <= 1e-8


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _nothing_after_a_bad_status():
    stopped = insts._stopped or vtrain._stopped
    if stopped:
        pytest.fail("not run: an earlier launch ended with %s" % (stopped[0],))


def _batch(inst, dev):
    cus = _cus(dev)
    n = sizes_batch(inst, cus)
    assert sizes_rule(n, inst[0], cus) == inst, (inst, n, cus)                                      # admitted, at C columns
    if n % 8 in (1, 2, 3, 4):
        assert columns_from_bytes(n, inst[0], _lib.lib().tk_gru_workspace_bytes(n, inst[0], cus)) == inst[1], (inst, n, cus)
    else:
        assert _lib.lib().tk_gru_workspace_bytes(n, inst[0], cus) == train_bytes(n, inst[0], inst[1])
    return n


def _inputs(H, N, T, dev):
    """tests/test_rnn_instantiations.py's GRU case (the layer at its own initialisation with a live bias_hh, its input,
    the float64 y) and what the kernels take: gx = x W_ih^T + b_ih, W_hh and b_hh on the device."""
    gru, x, ref = insts._gru_case(H, N, T)
    rnn = gru.rnn
    w_ih, w_hh = rnn.weight_ih_l0.detach().to(dev), rnn.weight_hh_l0.detach().to(dev).contiguous()
    b_hh = rnn.bias_hh_l0.detach().to(dev).contiguous()
    assert float(b_hh.abs().min()) > 0
    gx = (x.to(dev) @ w_ih.t() + rnn.bias_ih_l0.detach().to(dev)).contiguous()
    return gru, x, ref, gx, w_hh, b_hh


@functools.lru_cache(maxsize=None)
def _saved64(H, N, T):
    """y, gates and q of the float64 layer from x, both directions (computed once); y is `_gru_case`'s."""
    gru, x, ref = insts._gru_case(H, N, T)
    w_ih, w_hh, b_ih, b_hh = insts._params64(gru.rnn)
    out = {rev: _gru64(x.double() @ w_ih.t() + b_ih, w_hh, b_hh, None, rev) for rev in (0, 1)}
    for rev in (0, 1):
        assert (out[rev][0] - ref[rev][0]).abs().max().item() <= 1e-13
    return out


def _forward(gx, whh, bhh, rev, save=True):
    """tk_gru_forward_dev into guarded, sentinel-filled buffers (save False: NULL for gates and q); asserts the bounds,
    every element stored and finite; returns y, gates, q."""
    T, N, H3 = gx.shape
    H, dev, L = H3 // 3, gx.device, _lib.lib()
    wsb = L.tk_gru_workspace_bytes(N, H, _cus(dev))
    assert wsb > 0
    bufs = [rows._guarded(s, dev, 0) for s in ((T, N, H), (T, N, 3 * H), (T, N, H))]
    (_, y), (_, gates), (_, q) = bufs
    ws, status = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.tk_gru_forward_dev(_lib.ptr(gx), _lib.ptr(whh), _lib.ptr(bhh), T, N, H, rev, _cus(dev), _lib.ptr(y),
                              _lib.ptr(gates if save else None), _lib.ptr(q if save else None), _lib.ptr(ws), wsb,
                              _lib.ptr(status), _lib.stream_ptr())
    insts._finish(rc, status, "tk_gru_forward_dev")
    for name, (flat, body) in zip(("y", "gates", "q"), bufs):
        assert rows._guards_intact(flat, 0, body.numel()), (name, "a store outside the tensor")
        unwritten = int((body == rows.SENTINEL).sum().item())
        if save or name == "y":
            assert unwritten == 0, (name, "elements not stored", unwritten)
            assert bool(torch.isfinite(body).all()), name
        else:
            assert unwritten == body.numel(), (name, "written by the forward that saves nothing")
    return y, gates, q


def _backward(whh, y, gates, q, dy, rev):
    """tk_gru_backward_dev into guarded, sentinel-filled dgates and dq; asserts the bounds, returns both."""
    T, N, H = dy.shape
    dev, L = dy.device, _lib.lib()
    wsb = L.tk_gru_workspace_bytes(N, H, _cus(dev))
    assert wsb > 0
    (fg, dg), (fq, dq) = rows._guarded((T, N, 3 * H), dev, 0), rows._guarded((T, N, H), dev, 0)
    ws, status = torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)
    rc = L.tk_gru_backward_dev(_lib.ptr(whh), _lib.ptr(y), _lib.ptr(gates), _lib.ptr(q), _lib.ptr(dy), T, N, H, rev,
                               _cus(dev), _lib.ptr(dg), _lib.ptr(dq), _lib.ptr(ws), wsb, _lib.ptr(status),
                               _lib.stream_ptr())
    insts._finish(rc, status, "tk_gru_backward_dev")
    for name, flat, body in (("dgates", fg, dg), ("dq", fq, dq)):
        assert rows._guards_intact(flat, 0, body.numel()), (name, "a store outside the tensor")
        unwritten = int((body == rows.SENTINEL).sum().item())
        assert unwritten == 0, (name, "elements not stored", unwritten)
        assert bool(torch.isfinite(body).all()), name
    return dg, dq


_GRADS64 = {}


def _grads64(H, N, T, gx, w_hh, b_hh, lens=None):
    """`_pair64` on the kernel's own gx with insts._dy, both directions (computed once per shape)."""
    key = (H, N, T, lens is not None)
    if key not in _GRADS64:
        a = [v.detach().cpu().double() for v in (gx, w_hh, b_hh)]
        _GRADS64[key] = {rev: _pair64(*a, insts._dy(H, N, T).double(), lens, rev) for rev in (0, 1)}
    return _GRADS64[key]


def _miopen_dgates(gx, w_hh, b_hh, dy, rev):
    """MIOpen's dgates: the input gradient of nn.GRU(3H, H) with weight_ih = 1 and bias_ih = 0, fed gx."""
    H = w_hh.shape[1]
    m = torch.nn.GRU(3 * H, H).to(gx.device)
    with torch.no_grad():
        m.weight_ih_l0.copy_(torch.eye(3 * H))
        m.weight_hh_l0.copy_(w_hh)
        m.bias_ih_l0.zero_()
        m.bias_hh_l0.copy_(b_hh)
    xin = (torch.flip(gx, (0,)) if rev else gx).detach().clone().requires_grad_(True)
    (m(xin)[0] * (torch.flip(dy, (0,)) if rev else dy)).sum().backward()
    return torch.flip(xin.grad, (0,)) if rev else xin.grad


# --- 1. the saved tensors, dgates and dq at the C ABI ---------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_saved_tensors_match_float64_inside_their_bounds(gpu_device, inst, T, rev):
    H, n = inst[0], _batch(inst, gpu_device)
    gru, x, ref, gx, w_hh, b_hh = _inputs(H, n, T, gpu_device)
    got = _forward(gx, w_hh, b_hh, rev)                     # guarded, sentinel-filled: nothing outside, nothing unwritten
    e_mio = rows._rel(insts._miopen_gru_y(gru, x, rev, gpu_device), ref[rev][0])
    for name, a, r in zip(("y", "gates", "q"), got, _saved64(H, n, T)[rev]):
        e = rows._rel(a, r)
        print("gru fwd %s N %d T %d rev %d %s: error %.3e, MIOpen's y %.3e, ratio %.3f"
              % (_ids(inst), n, T, rev, name, e, e_mio, e / _allowed(e_mio)))
        assert r.abs().max().item() > 0 and e <= _allowed(e_mio), (inst, n, T, rev, name, e, e_mio)
    # NULL for the activations: the same y, bit for bit, and nothing else written
    assert torch.equal(_forward(gx, w_hh, b_hh, rev, save=False)[0], got[0])


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_backward_dgates_and_dq_match_float64_inside_their_bounds(gpu_device, inst, T, rev):
    H, n = inst[0], _batch(inst, gpu_device)
    _, _, _, gx, w_hh, b_hh = _inputs(H, n, T, gpu_device)
    y, gates, q = _forward(gx, w_hh, b_hh, rev)
    dy = insts._dy(H, n, T).to(gpu_device)
    dg, dq = _backward(w_hh, y, gates, q, dy, rev)
    ref = _grads64(H, n, T, gx, w_hh, b_hh)[rev]
    e_mio = rows._rel(_miopen_dgates(gx, w_hh, b_hh, dy, rev), ref["dgates"])
    for name, a in (("dgates", dg), ("dq", dq)):
        e = rows._rel(a, ref[name])
        print("gru bwd %s N %d T %d rev %d %s: error %.3e, MIOpen's dgates %.3e, ratio %.3f"
              % (_ids(inst), n, T, rev, name, e, e_mio, e / _allowed(e_mio)))
        assert ref[name].abs().max().item() > 0 and e <= _allowed(e_mio), (inst, n, T, rev, name, e, e_mio)


# --- 2. the layer, forward and backward -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_layer_matches_float64(gpu_device, inst, reverse):
    """GruMod and Reverse(GruMod), y and the five gradients (x, W_ih, W_hh, b_ih and a live b_hh) through
    tests/test_gru_hip.py's comparison.  T = 37: the step parity of every double buffer turns over many times, and most
    stores are the late ones."""
    H, n = inst[0], _batch(inst, gpu_device)
    test_gru_hip._compare(37, n, H, 20, reverse, gpu_device, seed=inst[1], live_bias_hh=True)
    _lib.raise_if_nonfinite()


# --- 3. the variable-length forms -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_varlen_inference_matches_masked_float64(gpu_device, inst, T, rev):
    """tk_gru_forward_varlen_dev (nothing saved): the masked float64 recurrence, exact zeros at and beyond the lengths,
    gx beyond them never used, and lengths = NULL / [T] * N the saving forward bit for bit."""
    H, n = inst[0], _batch(inst, gpu_device)
    gru, x, ref, gx, w_hh, b_hh = _inputs(H, n, T, gpu_device)
    e_mio = rows._rel(insts._miopen_gru_y(gru, x, rev, gpu_device), ref[rev][0])
    insts._check_varlen("gru", "gru VL %s N %d T %d rev %d" % (_ids(inst), n, T, rev), gx, w_hh, b_hh,
                        insts.lengths_for(n, T), rev, ref[rev][1], e_mio, lambda: varlen._gru_saving(gx, w_hh, b_hh, rev))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_varlen_training_pair_matches_masked_float64(gpu_device, inst, rev):
    """tk_gru_forward_varlen_save_dev / tk_gru_backward_varlen_dev with lengths_for (0, 1, T - 1 and T among them): y,
    gates, q, dgates and dq against the masked float64 recurrence on the kernel's own gx, MIOpen's full-length errors
    the allowance; all five exactly 0 at and beyond a length."""
    H, T, n = inst[0], 7, _batch(inst, gpu_device)
    dev = gpu_device
    gru, x, ref, gx, w_hh, b_hh = _inputs(H, n, T, dev)
    lens, dy = insts.lengths_for(n, T), insts._dy(H, n, T).to(dev)
    assert {0, 1, T - 1, T} <= set(lens)
    got = vtrain._pair("gru", gx, w_hh, b_hh, dy, lens, rev, train=True)
    beyond = torch.arange(T, device=dev)[:, None] >= torch.tensor(lens, device=dev)[None, :]
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (k, "a non-finite value")
        assert not v[beyond].any(), (k, "rows at and beyond the length are not exactly 0")
    want = _grads64(H, n, T, gx, w_hh, b_hh, lens)[rev]
    e_y = rows._rel(insts._miopen_gru_y(gru, x, rev, dev), ref[rev][0])
    e_dg = rows._rel(_miopen_dgates(gx, w_hh, b_hh, dy, rev), _grads64(H, n, T, gx, w_hh, b_hh)[rev]["dgates"])
    assert set(got) == set(want)
    for k, r in want.items():
        e, e_mio = rows._rel(got[k], r), e_dg if k in ("dgates", "dq") else e_y
        print("gru VL pair %s N %d rev %d %s: error %.3e, MIOpen's %.3e, ratio %.3f"
              % (_ids(inst), n, rev, k, e, e_mio, e / _allowed(e_mio)))
        assert r.abs().max().item() > 0 and e <= _allowed(e_mio), (inst, rev, k, e, e_mio)


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_varlen_training_columns_equal_the_column_run_alone(gpu_device, inst, rev):
    """... and every sampled column's rows are what the existing pair gives on that column alone over its own length
    (bit for bit where the launch at one column has the same (U, C): the 4-column forms; NaN in gx and dy beyond the
    lengths)."""
    H, T, n = inst[0], 7, _batch(inst, gpu_device)
    lens = insts.lengths_for(n, T)
    exact = sizes_rule(1, H, _cus(gpu_device)) == inst
    assert exact == (inst[1] == 4)
    gx, whh, bhh, dy = vtrain._abi_case("gru", H, n, T, gpu_device, 600 + H + rev)
    cols = vtrain._sample(n)
    assert {lens[c] for c in cols} == set(lens)
    vtrain._check_columns_alone("gru", gx, whh, bhh, dy, lens, rev, cols, exact, "gru %s rev %d" % (_ids(inst), rev))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_full_lengths_are_the_fixed_length_pair_bit_for_bit(gpu_device, inst, rev):
    H, n = inst[0], _batch(inst, gpu_device)
    for T in STEPS:
        gx, whh, bhh, dy = vtrain._abi_case("gru", H, n, T, gpu_device, 500 + H + 10 * T + rev)
        want = vtrain._pair("gru", gx, whh, bhh, dy, None, rev, train=False)
        for lens in (None, [T] * n):
            got = vtrain._pair("gru", gx, whh, bhh, dy, lens, rev, train=True)
            assert set(got) == set(want) == {"y", "gates", "c", "dgates", "dq"}
            for k in want:
                assert bool(torch.isfinite(want[k]).all()), (inst, T, k)
                assert torch.equal(got[k], want[k]), (inst, T, rev, "NULL" if lens is None else "[T] * N", k)


# --- 4. reproducibility ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_two_launches_give_the_same_bits(gpu_device, inst, rev):
    """Forward and backward: every sum runs in a fixed order (the backward's reduce-scatter in producer order)."""
    H, T, n = inst[0], 7, _batch(inst, gpu_device)
    _, _, _, gx, w_hh, b_hh = _inputs(H, n, T, gpu_device)
    a, b = _forward(gx, w_hh, b_hh, rev), _forward(gx, w_hh, b_hh, rev)
    for name, p, q in zip(("y", "gates", "q"), a, b):
        assert torch.equal(p, q), name
    dy = insts._dy(H, n, T).to(gpu_device)
    for p, q in zip(_backward(w_hh, *a, dy, rev), _backward(w_hh, *a, dy, rev)):
        assert torch.equal(p, q)


@pytest.mark.gpu
def test_captured_forward_replays_bit_identical(gpu_device):
    torch.manual_seed(7)
    layer = layers.Serial([layers.Reverse(layers.GruMod(32, 192)), layers.GruMod(192, 384)]).to(gpu_device)
    x = torch.randn(30, 21, 32, device=gpu_device)
    assert all(layers.hip_gru_workspace_bytes(m.rnn, x) > 0 for m in layer.modules() if isinstance(m, layers.GruMod))
    strict = _lib.is_strict()
    _lib.set_strict(False)
    try:
        with torch.no_grad():
            before = dict(layers.gru_forward_calls)
            eager = layer(x)
            assert layers.gru_forward_calls == dict(before, inference=before["inference"] + 2)
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


# --- 5. the models ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("net_kind,size", [("flipflop", 384), ("cat_mod", 192)])
def test_model_loss_and_gradients_match_the_fallback(gpu_device, net_kind, size):
    """One calculate_loss + backward of the reference's GRU model at the trainer's default size (and of the cat-mod twin
    at 192), chunk_len 200 at the trainer's stride 5 (T = 40), N = 5: every GRU layer runs the HIP recurrence, and the
    loss and every parameter gradient are as close to the float64 model as 2 x the nn.GRU path's own error + 2e-6."""
    from taiyaki_amd import models
    torch.manual_seed(size)
    make = models.mGru_flipflop if net_kind == "flipflop" else models.mGru_cat_mod_flipflop
    net = make(size=size, stride=5).to(gpu_device)
    batch = lstm_sizes._model_batch(net_kind, 200, 5, gpu_device)
    grus = [m for m in net.modules() if isinstance(m, layers.GruMod)]
    probe = torch.zeros(40, 5, size, device=gpu_device)
    assert len(grus) == 5 and all(layers.hip_gru_workspace_bytes(m.rnn, probe) > 0 for m in grus)
    before = dict(layers.gru_forward_calls)
    hip = lstm_sizes._loss_and_grads(net, batch)
    assert layers.gru_forward_calls == dict(before, saved=before["saved"] + 5), "a GRU layer did not take the HIP path"
    old = layers.USE_HIP_GRU
    try:
        layers.USE_HIP_GRU = False
        assert all(layers.hip_gru_workspace_bytes(m.rnn, probe) == 0 for m in grus)
        fallback = lstm_sizes._loss_and_grads(net, batch)
        assert layers.gru_forward_calls == dict(before, saved=before["saved"] + 5)
    finally:
        layers.USE_HIP_GRU = old
    _lib.raise_if_nonfinite()
    ref = lstm_sizes._float64_loss_and_grads(net, batch, gpu_device)
    assert set(ref) == set(hip) == set(fallback) and sum(".rnn." in k for k in ref) == 15 and "loss" in ref
    for k, r in ref.items():
        scale = r.abs().max().item() or 1.0
        e_hip, e_fb = (hip[k] - r).abs().max().item() / scale, (fallback[k] - r).abs().max().item() / scale
        print("%s %d %s: HIP %.3e, nn.GRU %.3e, ratio %.3f" % (net_kind, size, k, e_hip, e_fb, e_hip / _allowed(e_fb)))
        assert e_hip <= _allowed(e_fb), (net_kind, size, k, e_hip, e_fb)


@pytest.mark.gpu
def test_basecaller_short_reads_call_the_same_sequences_as_the_fallback(gpu_device):
    """Basecaller(batch_short=True) on three reads shorter than a chunk, at size 192: the same sequences from the HIP
    recurrence (variable-length columns) and from nn.GRU.  The two paths' scores differ by float32 rounding, so a call
    could differ where two paths through the trellis are closer than that; such a difference is acceptable only where
    both paths' scores differ from the float64 model's by less than their gap at that position, and is to be shown by
    inspecting the scores, not assumed.  With these seeds the calls are equal."""
    from taiyaki_amd import basecall, models, synth
    torch.manual_seed(15)
    net = synth.excite_network(models.mGru_flipflop(size=192, stride=5)).to(gpu_device).eval()
    rs = np.random.RandomState(4)
    sigs = [(90 + 12 * rs.standard_normal(n) + 3 * np.sin(np.arange(n) / 50.0)).astype(np.float32) for n in (400, 333, 777)]
    before = dict(layers.rnn_varlen_calls)
    calls = basecall.Basecaller(net, stride=5, chunk_size=200, overlap=20, batch_short=True).call(sigs)
    assert layers.rnn_varlen_calls["inference"] > before["inference"], "the short reads did not take the HIP recurrence"
    old = layers.USE_HIP_GRU
    try:
        layers.USE_HIP_GRU = False
        fallback = basecall.Basecaller(net, stride=5, chunk_size=200, overlap=20, batch_short=True).call(sigs)
    finally:
        layers.USE_HIP_GRU = old
    _lib.raise_if_nonfinite()
    assert [c[2] for c in calls] == [400, 333, 777] and all(len(c[0]) > 0 and set(c[0]) <= set("ACGT") for c in calls)
    assert [c[0] for c in calls] == [c[0] for c in fallback]
