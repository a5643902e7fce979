"""The LSTM recurrence at hidden sizes 192 and 384 (csrc/lstm_kernels.hip): the sizes that are no power of two.

The rule under test (lstm_geometry / lstm_plan).  A workgroup owns U = 48 hidden units, a group is G = H / 48 workgroups
that share C batch columns.  C = 4 where ceil(N / 4) * G <= CUs; else, at H = 192 only, C = 8 where ceil(N / 8) * G <= CUs;
else the batch is refused (the forward at (384, 48, 8) does not fit its registers, so that instantiation does not exist).
On 256 CUs: H = 384 takes N <= 128, H = 192 takes N <= 512 (4 columns up to 256).  The workspace is the backward's
granules, 2 slots x groups x G producers x C x H x 8 bytes, and bounds the forward's.

An instantiation is named (H, U, C), as in tests/test_rnn_instantiations.py, whose helpers, references and allowance this
file imports: error over the tensor's largest entry <= 2 x MIOpen's own + 2e-6, both against float64.  The batches follow
`lstm_batch`: 7 C + 1 columns for the first column count (8 groups, the last ragged), one column more than the first
count admits on the device for the second (257 at H = 192 on 256 CUs).

Every launch at the C ABI asserts return code 0 and status word 0 behind the synchronise; after a non-zero status of
this file's launches nothing more is launched (the remaining tests fail at once)."""
import copy
import ctypes

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, layers
from tests import test_lstm_fwd_rows as rows, test_lstm_hip, test_rnn_entry_checks as entry
from tests import test_rnn_instantiations as insts, test_rnn_varlen as varlen, test_rnn_varlen_train as vtrain

SIZES = (192, 384)
NEW_INSTS = [(192, 48, 4), (192, 48, 8), (384, 48, 4)]
FIRST = [i for i in NEW_INSTS if i[2] == 4]              # the first column count of each size
STEPS = insts.STEPS
_ids = insts._ids
_cus = rows._cus
_allowed = insts._allowed


# ---------------------------------------------------------------------------------------------------------------------
# the rule, restated
# ---------------------------------------------------------------------------------------------------------------------
def columns_of(h):
    return (4, 8) if h == 192 else (4,)


def sizes_rule(n, h, cus):
    if h not in SIZES or n <= 0 or cus <= 0:
        return None
    for c in columns_of(h):
        if -(-n // c) * (h // 48) <= cus:
            return (h, 48, c)
    return None


def last_admitted(h, cus):
    return columns_of(h)[-1] * (cus // (h // 48))


def sizes_batch(inst, cus):
    h, _, c = inst
    if c == columns_of(h)[0]:
        return 7 * c + 1
    return columns_of(h)[0] * (cus // (h // 48)) + 1     # one column more than the first count admits


def _geometry(L, n, h, cus):
    out = (ctypes.c_size_t * 8)()
    return [int(v) for v in out] if L.tk_lab_lstm_geometry(n, h, cus, out) else None


# ---------------------------------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------------------------------
def test_workspace_query_admits_the_two_sizes_and_refuses_the_rest():
    ws = _lib.lib().tk_lstm_workspace_bytes
    assert ws(128, 384, 256) == 2 * 32 * 8 * 4 * 384 * 8         # 32 groups of 8 workgroups, 4 columns: the 256 CUs
    assert ws(256, 192, 256) == 2 * 64 * 4 * 4 * 192 * 8         # 64 groups of 4 workgroups, 4 columns
    assert ws(257, 192, 256) == 2 * 33 * 4 * 8 * 192 * 8         # 8 columns
    for h in SIZES:
        assert ws(1, h, 256) > 0 and ws(1, h, h // 48) > 0
        assert ws(0, h, 256) == 0 and ws(128, h, 0) == 0 and ws(1, h, h // 48 - 1) == 0
        for cus in (256, 64):
            assert ws(last_admitted(h, cus), h, cus) > 0 and ws(last_admitted(h, cus) + 1, h, cus) == 0, (h, cus)
    assert (last_admitted(384, 256), last_admitted(192, 256)) == (128, 512)
    for h in (96, 512, 48, 144, 240, 288, 576, 768):
        assert ws(128, h, 256) == 0 and ws(1, h, 256) == 0, h


def test_rule_is_the_librarys_plan_for_every_batch():
    V, T = _lib.varlen_lib(), _lib.varlen_train_lib()
    kind = _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"]
    ws = _lib.lib().tk_lstm_workspace_bytes
    L = _lib.use_lab(True)
    try:
        L.tk_lab_lstm_units(0)
        seen = set()
        for cus in (256, 64):
            for h in SIZES:
                G = h // 48
                for n in range(1, last_admitted(h, cus) + 2):
                    want, got = sizes_rule(n, h, cus), _geometry(L, n, h, cus)
                    assert (want is None) == (got is None) == (n > last_admitted(h, cus)), (n, h, cus)
                    # the three libraries admit exactly the same (N, H, CUs)
                    q = ws(n, h, cus)
                    assert (q > 0) == (V.tk_rnn_varlen_workspace_bytes(kind, n, h, cus) > 0) \
                        == (T.tk_rnn_varlen_train_workspace_bytes(kind, n, h, cus) > 0) == (want is not None), (n, h, cus)
                    if want is None:
                        continue
                    c, groups = want[2], -(-n // want[2])
                    # admitted columns and groups, then the plan: U, C, groups, grid, forward and backward granule bytes
                    assert got == [c, groups, 48, c, groups, groups * G, 2 * groups * c * h * 8, 2 * groups * G * c * h * 8]
                    assert got[5] <= cus, "one workgroup per CU: the members of a group wait on each other"
                    assert got[6] <= got[7] == q == T.tk_rnn_varlen_train_workspace_bytes(kind, n, h, cus)
                    assert V.tk_rnn_varlen_workspace_bytes(kind, n, h, cus) == got[6]
                    seen.add(want)
        assert seen == set(NEW_INSTS)
        # the lab's forced units are those of the power-of-two sizes: they do not apply
        for u in (16, 32, 64):
            L.tk_lab_lstm_units(u)
            assert _geometry(L, 29, 384, 256)[2:4] == [48, 4] and _geometry(L, 257, 192, 256)[2:4] == [48, 8]
    finally:
        L.tk_lab_lstm_units(0)
        _lib.use_lab(False)


@pytest.mark.parametrize("cus", [256, 64])
def test_batches_select_their_instantiation_ragged(cus):
    for inst in NEW_INSTS:
        n = sizes_batch(inst, cus)
        assert insts._lab_lstm_inst(n, inst[0], cus) == inst == sizes_rule(n, inst[0], cus), (inst, n)
        assert n % inst[2] != 0 and -(-n // inst[2]) >= 3, (inst, n)
        insts._every_position_meets_every_length(n, inst[2])
    assert insts._lab_lstm_inst(sizes_batch((192, 48, 8), cus) - 1, 192, cus) == (192, 48, 4)
    assert [sizes_batch(i, 256) for i in NEW_INSTS] == [29, 257, 29]


LSTM_ENTRIES = [name for name, v in entry.ENTRIES.items() if v[1] == "lstm"]


@pytest.mark.parametrize("shape", [(5, 192, 256), (257, 192, 256), (5, 384, 256), (128, 384, 256)], ids=_ids)
@pytest.mark.parametrize("name", LSTM_ENTRIES)
def test_entries_check_the_workspace_at_the_new_sizes(name, shape):
    """tests/test_rnn_entry_checks.py's calls (fake pointers that are never dereferenced: every answer comes before any
    HIP call): the last byte of the launch's own need is missed, forward and backward, in all three libraries."""
    assert len(LSTM_ENTRIES) == 5
    e = entry.Entry(name, shape)
    assert 0 < e.need <= e.query and e.need % 16 == 0
    assert e() == entry.WORKSPACE
    assert e(workspace_bytes=e.need - 1) == entry.WORKSPACE
    assert e(nblk=0, workspace_bytes=e.need - 1) == entry.WORKSPACE
    assert e(nblk=0, workspace_bytes=e.need) == entry.OK
    assert e(nbatch=last_admitted(shape[1], shape[2]) + 1) == entry.UNSUPPORTED     # the plan is asked before the workspace
    assert e(workspace=None) == entry.BAD_ARG


def test_masked_float64_reference_is_differentiable():
    """The variable-length backward's reference, before it judges a kernel: the gradient of the masked float64 recurrence
    of tests/test_rnn_instantiations.py is, column by column, that of the column run alone over its own length, and
    exactly 0 at and beyond it."""
    H, N, T = 8, 9, 7
    g = torch.Generator().manual_seed(5)
    gx, w_hh = torch.randn(T, N, 4 * H, generator=g).double(), torch.randn(4 * H, H, generator=g).double() / H ** 0.5
    dy, lens = torch.randn(T, N, H, generator=g).double(), insts.lengths_for(N, T)
    for rev in (0, 1):
        y, dg = _masked_pair64(gx, w_hh, dy, lens, rev)
        for n in range(N):
            ln = lens[n]
            assert not dg[ln:, n].any() and not y[ln:, n].any()
            if ln:
                a = gx[:ln, n:n + 1].clone().requires_grad_(True)
                eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, dtype=torch.float64)
                (rows._float64_lstm(a, eye, w_hh, zero, rev)[0] * dy[:ln, n:n + 1]).sum().backward()
                assert (a.grad[:, 0] - dg[:ln, n]).abs().max().item() <= 1e-13


def _masked_pair64(gx64, w_hh64, dy64, lens, rev):
    """y and d (y * dy).sum() / d gx of the masked float64 recurrence on pre-activations gx."""
    H = w_hh64.shape[1]
    eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, dtype=torch.float64)
    g = gx64.detach().clone().requires_grad_(True)
    y = insts._masked_lstm(g, eye, w_hh64, zero, lens, rev)
    (y * dy64).sum().backward()
    return y.detach(), g.grad.detach()


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(autouse=True)
def _nothing_after_a_bad_status():
    stopped = insts._stopped or vtrain._stopped
    if stopped:
        pytest.fail("not run: an earlier launch ended with %s" % (stopped[0],))


def _batch(inst, dev):
    n = sizes_batch(inst, _cus(dev))
    assert insts._lab_lstm_inst(n, inst[0], _cus(dev)) == inst, (inst, n, _cus(dev))
    return n


# --- 1. the layer, forward and backward -----------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("wide_input", [False, True], ids=["I7", "IH"])
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_layer_matches_float64(gpu_device, inst, wide_input, reverse):
    """layers.Lstm forward and backward (y, dx, dW_ih, dW_hh, db) through tests/test_lstm_hip.py's comparison."""
    H, n = inst[0], _batch(inst, gpu_device)
    test_lstm_hip._compare(5, n, H, H if wide_input else 7, reverse, gpu_device, seed=inst[2])
    _lib.raise_if_nonfinite()


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T", [1, 2, 37])
@pytest.mark.parametrize("inst", FIRST, ids=_ids)
def test_layer_matches_float64_at_the_edges_and_over_many_steps(gpu_device, inst, T, reverse):
    """T = 1: the epilogue's stores alone, no hand-off.  T = 2: one deferred store, one granule hand-off.  T = 37: the
    step parity of every double buffer turns over many times."""
    H, n = inst[0], _batch(inst, gpu_device)
    test_lstm_hip._compare(T, n, H, 7, reverse, gpu_device, seed=T)
    _lib.raise_if_nonfinite()


# --- 2. the saved tensors and dgates at the C ABI -------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_saved_tensors_match_float64_inside_their_bounds(gpu_device, inst, T, rev):
    H, n = inst[0], _batch(inst, gpu_device)
    rnn, x, ref, gx, w_hh = rows._inputs(H, n, T, gpu_device)
    got = rows._forward(gx, w_hh, rev)                      # guarded, sentinel-filled: nothing outside, nothing unwritten
    e_mio = rows._rel(rows._miopen_y(rnn, x, rev, gpu_device), ref[rev][0])
    for name, a, r in zip(("y", "gates", "cell"), got, ref[rev]):
        e = rows._rel(a, r)
        print("lstm fwd %s N %d T %d rev %d %s: error %.3e, MIOpen's y %.3e, ratio %.3f"
              % (_ids(inst), n, T, rev, name, e, e_mio, e / _allowed(e_mio)))
        assert e <= _allowed(e_mio), (inst, n, T, rev, name, e, e_mio)


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_backward_dgates_match_float64_inside_their_bounds(gpu_device, inst, T, rev):
    H, n = inst[0], _batch(inst, gpu_device)
    _, _, _, gx, w_hh = rows._inputs(H, n, T, gpu_device)
    _, gates, cell = rows._forward(gx, w_hh, rev)
    dy = insts._dy(H, n, T).to(gpu_device)
    dg = insts._backward(w_hh, gates, cell, dy, rev)
    ref = insts._dgates64(H, n, T, gx, w_hh)[rev]
    assert ref.abs().max().item() > 0
    e, e_mio = rows._rel(dg, ref), rows._rel(insts._miopen_dgates(gx, w_hh, dy, rev), ref)
    print("lstm bwd %s N %d T %d rev %d dgates: error %.3e, MIOpen's %.3e, ratio %.3f"
          % (_ids(inst), n, T, rev, e, e_mio, e / _allowed(e_mio)))
    assert e <= _allowed(e_mio), (inst, n, T, rev, e, e_mio)


# --- 3. the variable-length forms -----------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_varlen_inference_matches_masked_float64(gpu_device, inst, T, rev):
    """tk_lstm_forward_varlen_dev (nothing saved): the masked float64 recurrence, exact zeros at and beyond the lengths,
    gx beyond them never used, and lengths = NULL / [T] * N the saving forward bit for bit."""
    H, n = inst[0], _batch(inst, gpu_device)
    rnn, x, ref, gx, w_hh = rows._inputs(H, n, T, gpu_device)
    e_mio = rows._rel(rows._miopen_y(rnn, x, rev, gpu_device), ref[rev][0])
    insts._check_varlen("lstm", "lstm VL %s N %d T %d rev %d" % (_ids(inst), n, T, rev), gx, w_hh, None,
                        insts.lengths_for(n, T), rev, insts._lstm_masked64(H, n, T)[rev], e_mio,
                        lambda: varlen._lstm_saving(gx, w_hh, rev))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_varlen_training_pair_matches_masked_float64(gpu_device, inst, rev):
    """tk_lstm_forward_varlen_save_dev / tk_lstm_backward_varlen_dev with lengths_for (0, 1, T - 1 and T among them): y
    and dgates against the masked float64 recurrence on the kernel's own gx, MIOpen's full-length errors the allowance;
    y, the gates, c and dgates exactly 0 at and beyond a length."""
    H, T, n = inst[0], 7, _batch(inst, gpu_device)
    dev = gpu_device
    rnn, x, ref, gx, w_hh = rows._inputs(H, n, T, dev)
    lens, dy = insts.lengths_for(n, T), insts._dy(H, n, T).to(dev)
    assert {0, 1, T - 1, T} <= set(lens)
    got = vtrain._pair("lstm", gx, w_hh, None, dy, lens, rev, train=True)
    beyond = torch.arange(T, device=dev)[:, None] >= torch.tensor(lens, device=dev)[None, :]
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (k, "a non-finite value")
        assert not v[beyond].any(), (k, "rows at and beyond the length are not exactly 0")
    y64, dg64 = _masked_pair64(gx.detach().cpu().double(), w_hh.detach().cpu().double(), dy.cpu().double(), lens, rev)
    e_mio = {"y": rows._rel(rows._miopen_y(rnn, x, rev, dev), ref[rev][0]),
             "dgates": rows._rel(insts._miopen_dgates(gx, w_hh, dy, rev), insts._dgates64(H, n, T, gx, w_hh)[rev])}
    for k, r in (("y", y64), ("dgates", dg64)):
        e = rows._rel(got[k], r)
        print("lstm VL pair %s N %d rev %d %s: error %.3e, MIOpen's %.3e, ratio %.3f"
              % (_ids(inst), n, rev, k, e, e_mio[k], e / _allowed(e_mio[k])))
        assert r.abs().max().item() > 0 and e <= _allowed(e_mio[k]), (inst, rev, k, e, e_mio[k])


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_varlen_training_columns_equal_the_column_run_alone(gpu_device, inst, rev):
    """... and every sampled column's rows are what the existing pair gives on that column alone over its own length
    (bit for bit where the launch at one column has the same (U, C); NaN in gx and dy beyond the lengths)."""
    H, T, n = inst[0], 7, _batch(inst, gpu_device)
    lens = insts.lengths_for(n, T)
    exact = varlen._lstm_same_geometry(n, H, _cus(gpu_device))
    assert exact == (inst[2] == 4)
    gx, whh, bhh, dy = vtrain._abi_case("lstm", H, n, T, gpu_device, 600 + H + rev)
    cols = vtrain._sample(n)
    assert {lens[c] for c in cols} == set(lens)
    vtrain._check_columns_alone("lstm", gx, whh, bhh, dy, lens, rev, cols, exact, "lstm %s rev %d" % (_ids(inst), rev))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", NEW_INSTS, ids=_ids)
def test_full_lengths_are_the_fixed_length_pair_bit_for_bit(gpu_device, inst, rev):
    H, n = inst[0], _batch(inst, gpu_device)
    for T in STEPS:
        gx, whh, bhh, dy = vtrain._abi_case("lstm", H, n, T, gpu_device, 500 + H + 10 * T + rev)
        want = vtrain._pair("lstm", gx, whh, bhh, dy, None, rev, train=False)
        for lens in (None, [T] * n):
            got = vtrain._pair("lstm", gx, whh, bhh, dy, lens, rev, train=True)
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
    _, _, _, gx, w_hh = rows._inputs(H, n, T, gpu_device)
    a, b = rows._forward(gx, w_hh, rev), rows._forward(gx, w_hh, rev)
    for name, p, q in zip(("y", "gates", "cell"), a, b):
        assert torch.equal(p, q), name
    dy = insts._dy(H, n, T).to(gpu_device)
    assert torch.equal(insts._backward(w_hh, a[1], a[2], dy, rev), insts._backward(w_hh, a[1], a[2], dy, rev))


@pytest.mark.gpu
def test_captured_forward_replays_bit_identical(gpu_device):
    torch.manual_seed(7)
    layer = layers.Serial([layers.Reverse(layers.Lstm(32, 192)), layers.Lstm(192, 192)]).to(gpu_device)
    x = torch.randn(30, 21, 32, device=gpu_device)
    assert all(layers.hip_lstm_workspace_bytes(m.rnn, x) > 0 for m in layer.modules() if isinstance(m, layers.Lstm))
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


# --- 5. the weight gradients -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("inst", FIRST, ids=_ids)
def test_weight_gradient_kernel_agrees_with_the_gemms(gpu_device, inst, reverse):
    """tk_lstm_weight_grad_dev at I = H (384 = 3 x 128: its aligned kernel; 192: the general one) on the dG of the new
    recurrences, against the two GEMMs and the sum (layers.USE_HIP_LSTM_WGRAD off), both against float64."""
    H, T, n = inst[0], 5, _batch(inst, gpu_device)
    assert _lib.wgrad_lib().tk_lstm_weight_grad_workspace_bytes(T, n, H, H, _cus(gpu_device)) > 0
    torch.manual_seed(40 + H)
    lstm = layers.Lstm(H, H)
    layer = layers.Reverse(lstm) if reverse else lstm
    x, dy = torch.randn(T, n, H), torch.randn(T, n, H) / (T * n) ** 0.5
    ref = test_lstm_hip._grads(layer.double(), x.double(), dy.double())
    layer = layer.float().to(gpu_device)
    assert layers.hip_lstm_workspace_bytes(lstm.rnn, x.to(gpu_device)) > 0
    old = layers.USE_HIP_LSTM_WGRAD
    try:
        layers.USE_HIP_LSTM_WGRAD = True
        fused = test_lstm_hip._grads(layer, x.to(gpu_device), dy.to(gpu_device))
        layers.USE_HIP_LSTM_WGRAD = False
        gemm = test_lstm_hip._grads(layer, x.to(gpu_device), dy.to(gpu_device))
    finally:
        layers.USE_HIP_LSTM_WGRAD = old
    _lib.raise_if_nonfinite()
    for k in ("w_ih", "w_hh", "b_ih"):
        e_fused, e_gemm = rows._rel(fused[k], ref[k]), rows._rel(gemm[k], ref[k])
        print("%s rev %d d%s: fused %.3e, GEMMs %.3e" % (_ids(inst), reverse, k, e_fused, e_gemm))
        assert e_fused <= _allowed(e_gemm), (inst, k, e_fused, e_gemm)


# --- 6. the models ---------------------------------------------------------------------------------------------------
def _model_batch(net_kind, T_chunk, N, dev):
    from taiyaki_amd import synth
    sl = synth.realistic_seqlens(T_chunk // 5, N, 8, T_chunk, 9.0)
    sq, bases = synth.sequences(sl, 8)
    batch = dict(indata=torch.from_numpy(synth.signal_chunks(T_chunk, N, 8)).to(dev), seqs=torch.from_numpy(sq),
                 seqlens=torch.from_numpy(sl))
    if net_kind == "cat_mod":
        batch.update(mod_cats=torch.from_numpy(synth.mod_cats(bases, 8, (1, 1, 0, 0))),
                     can_mods_offsets=synth.can_mods_offsets((1, 1, 0, 0)),
                     mod_cat_weights=np.full(6, 8.0, dtype=np.float32))
    return batch


def _loss_and_grads(net, batch):
    from taiyaki_amd import train
    for p in net.parameters():
        p.grad = None
    loss = train.calculate_loss(net, **batch)[0]
    loss.backward()
    out = {k: p.grad.detach().double().cpu() for k, p in vtrain._named(net)}       # (bias_hh is frozen at 0)
    out["loss"] = loss.detach().double().cpu().reshape(1)
    return out


def _float64_loss_and_grads(net, batch, dev):
    """The float64 copy of the model on the CPU up to its scores; the loss, which is not under test and is the same
    operator on both paths, is the project's own on those scores rounded to float32 (one rounding, 6e-8 relative), and
    its gradient goes back through the float64 network."""
    from taiyaki_amd import train
    n64 = copy.deepcopy(net).cpu().double()
    scores = n64(batch["indata"].cpu().double())

    class Scores(torch.nn.Module):
        def forward(self, _):
            return self.leaf

    head = Scores()
    head.leaf = scores.detach().float().to(dev).requires_grad_(True)
    loss = train.calculate_loss(head, **batch)[0]
    loss.backward()
    scores.backward(head.leaf.grad.double().cpu())
    out = {k: p.grad.detach() for k, p in vtrain._named(n64)}
    out["loss"] = loss.detach().double().cpu().reshape(1)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("net_kind,size", [("flipflop", 384), ("cat_mod", 192)])
def test_model_loss_and_gradients_match_the_fallback(gpu_device, net_kind, size):
    """One calculate_loss + backward of the reference's recommended model at its default size (and of the cat-mod twin
    at 192), chunk_len 200 (T = 40), N = 5: every LSTM layer runs the HIP recurrence, and the loss and every parameter
    gradient are as close to the float64 model as 2 x the nn.LSTM path's own error + 2e-6."""
    from taiyaki_amd import models
    torch.manual_seed(size)
    make = models.mLstm_flipflop if net_kind == "flipflop" else models.mLstm_cat_mod_flipflop
    net = make(size=size, stride=5).to(gpu_device)
    batch = _model_batch(net_kind, 200, 5, gpu_device)
    lstms = [m for m in net.modules() if isinstance(m, layers.Lstm)]
    probe = torch.zeros(40, 5, size, device=gpu_device)
    assert len(lstms) == 5 and all(layers.hip_lstm_workspace_bytes(m.rnn, probe) > 0 for m in lstms)
    hip = _loss_and_grads(net, batch)
    old = layers.USE_HIP_LSTM
    try:
        layers.USE_HIP_LSTM = False
        assert all(layers.hip_lstm_workspace_bytes(m.rnn, probe) == 0 for m in lstms)
        fallback = _loss_and_grads(net, batch)
    finally:
        layers.USE_HIP_LSTM = old
    _lib.raise_if_nonfinite()
    ref = _float64_loss_and_grads(net, batch, gpu_device)
    assert set(ref) == set(hip) == set(fallback) and len(ref) == 1 + 6 + 15 + 2
    for k, r in ref.items():
        scale = r.abs().max().item() or 1.0
        e_hip, e_fb = (hip[k] - r).abs().max().item() / scale, (fallback[k] - r).abs().max().item() / scale
        print("%s %d %s: HIP %.3e, nn.LSTM %.3e, ratio %.3f" % (net_kind, size, k, e_hip, e_fb, e_hip / _allowed(e_fb)))
        assert e_hip <= _allowed(e_fb), (net_kind, size, k, e_hip, e_fb)


@pytest.mark.gpu
def test_basecaller_short_reads_call_the_same_sequences_as_the_fallback(gpu_device):
    """Basecaller(batch_short=True) on three reads shorter than a chunk, at size 192: the same sequences from the HIP
    recurrence (variable-length columns) and from nn.LSTM.  The two paths' scores differ by float32 rounding, so a call
    could differ where two paths through the trellis are closer than that; such a difference is acceptable only where
    both paths' scores differ from the float64 model's by less than their gap at that position, and is to be shown by
    inspecting the scores, not assumed.  With these seeds the calls are equal."""
    from taiyaki_amd import basecall, models, synth
    torch.manual_seed(15)
    net = synth.excite_network(models.mLstm_flipflop(size=192, stride=5)).to(gpu_device).eval()
    rs = np.random.RandomState(4)
    sigs = [(90 + 12 * rs.standard_normal(n) + 3 * np.sin(np.arange(n) / 50.0)).astype(np.float32) for n in (400, 333, 777)]
    before = dict(layers.rnn_varlen_calls)
    calls = basecall.Basecaller(net, stride=5, chunk_size=200, overlap=20, batch_short=True).call(sigs)
    assert layers.rnn_varlen_calls["inference"] > before["inference"], "the short reads did not take the HIP recurrence"
    old = layers.USE_HIP_LSTM
    try:
        layers.USE_HIP_LSTM = False
        fallback = basecall.Basecaller(net, stride=5, chunk_size=200, overlap=20, batch_short=True).call(sigs)
    finally:
        layers.USE_HIP_LSTM = old
    _lib.raise_if_nonfinite()
    assert [c[2] for c in calls] == [400, 333, 777] and all(len(c[0]) > 0 and set(c[0]) <= set("ACGT") for c in calls)
    assert [c[0] for c in calls] == [c[0] for c in fallback]
