"""Training through batches whose columns differ in length: the saving forward and the backward with per-column
lengths (include/taiyaki_amd_rnn_varlen_train.h, libtaiyaki_amd_rnn_varlen_train.so) at the C ABI, `Lstm` / `GruMod`
`forward(x, reverse, lengths)` under grad mode, and `layers.forward_varlen` under grad mode.

The rule under test: where t >= lengths[n] every saved tensor, dgates and dq are exactly 0 and the step hands on a zero
recurrent gradient; otherwise the step is that of the existing training pair.  So a column's rows are what the column
gives run alone at its own length, and lengths = NULL is the existing training pair, bit for bit.

Every launch at the C ABI asserts return code 0 and status word 0 behind the synchronise; after a non-zero status this
module launches nothing more (the remaining tests fail at once).  Outputs are NaN before every launch."""
import copy
import ctypes
import functools
import os
import re
import subprocess

import pytest
import torch

from taiyaki_amd import _lib, layers, models
from tests import test_rnn_varlen as varlen
from tests.test_rnn_instantiations import (GRU_INSTS, LSTM_INSTS, STEPS, _ids, _lab_lstm_inst, gru_batch, gru_rule,
                                           lengths_for, lstm_batch)

@pytest.fixture(autouse=True)
def _train_varlen(monkeypatch):
    """Every test here trains through lengths: the switch is off by default (tests/test_forward_varlen.py holds that)."""
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)


# ---------------------------------------------------------------------------------------------------------------------
# shared: gradients of a call, and the per-column sums they are held against
# ---------------------------------------------------------------------------------------------------------------------
def _named(module):
    return [(k, p) for k, p in module.named_parameters() if p.requires_grad]


def _grads(module, call, x, dy):
    """y = call(x) and d (y * dy).sum() / d (x, every parameter of `module` that requires a gradient)."""
    x = x.detach().clone().requires_grad_(True)
    for _, p in _named(module):
        p.grad = None
    y = call(x)
    (y * dy).sum().backward()
    out = {"y": y, "x": x.grad}
    out.update({k: p.grad for k, p in _named(module)})
    return {k: v.detach().clone() for k, v in out.items()}


def _column_sums(module, call, x, dy, in_lens, out_lens, parts=False):
    """The same from every column run alone at its own length, accumulated in float64 on the CPU: y and dx column by
    column (0 beyond the lengths), the parameter gradients summed over the columns.  parts: also sum |term| per
    parameter (what bounds the rounding of a float32 sum of the same terms in any order)."""
    T, N = x.shape[:2]
    acc, mag = {}, {}
    for n in range(N):
        li, lo = int(in_lens[n]), int(out_lens[n])
        if li == 0:
            continue
        g = _grads(module, call, x[:li, n:n + 1].contiguous(), dy[:lo, n:n + 1].contiguous())
        if "y" not in acc:
            acc["y"] = torch.zeros((dy.shape[0], N) + tuple(g["y"].shape[2:]), dtype=torch.float64)
            acc["x"] = torch.zeros(tuple(x.shape), dtype=torch.float64)
        acc["y"][:lo, n:n + 1] = g["y"].double().cpu()
        acc["x"][:li, n:n + 1] = g["x"].double().cpu()
        for k, v in g.items():
            if k not in ("y", "x"):
                v = v.double().cpu()
                acc[k] = acc.get(k, 0) + v
                mag[k] = mag.get(k, 0) + v.abs()
    return (acc, mag) if parts else acc


def _err(a, ref):
    return (a.double().cpu() - ref).abs().max().item() / (ref.abs().max().item() or 1.0)


def _small_serial():
    """conv with stride 2 -> Lstm -> Reverse(GruMod) -> GlobalNormFlipFlop"""
    return layers.Serial([layers.Convolution(1, 8, 5, stride=2), layers.Lstm(8, 32),
                          layers.Reverse(layers.GruMod(32, 32)), layers.GlobalNormFlipFlop(32, 4)])


def _padded(T, lengths, seed, channels=1):
    x = torch.randn(T, len(lengths), channels, generator=torch.Generator().manual_seed(seed))
    for n, ln in enumerate(lengths):
        x[ln:, n] = 0
    return x


# ---------------------------------------------------------------------------------------------------------------------
# CPU 1: the fallback under grad mode
# ---------------------------------------------------------------------------------------------------------------------
CPU_T, CPU_LENS = 9, [9, 0, 1, 5]


def _assert_float32_sums(got, module, make_call, x, dy, in_lens, out_lens, what):
    """`got` (float32, the batched call) against every column alone in float64, by the project's rule with every column
    alone in float32 as the yardstick: err <= 2 err_alone + 2e-6, each error over the tensor's largest entry.  (The
    fallback runs the same per-column passes, on views of x instead of copies: nn.GRU's weight gradients then differ
    from the copies' in the last bits, so float32 rounding is measured, not assumed to cancel.)"""
    m64 = copy.deepcopy(module).double()
    ref = _column_sums(m64, make_call(m64), x.double(), dy.double(), in_lens, out_lens)
    alone = _column_sums(module, make_call(module), x, dy, in_lens, out_lens)
    _compare_with_columns_alone(ref, got, alone, what)
    beyond = torch.arange(dy.shape[0])[:, None] >= torch.as_tensor(out_lens)[None, :]
    assert not got["y"][beyond].any(), (what, "rows of y beyond the length")
    assert not got["x"][torch.arange(x.shape[0])[:, None] >= torch.as_tensor(in_lens)[None, :]].any(), (what, "dx")


def _compare_with_columns_alone(ref, batched, alone, what):
    """tests/test_lstm_hip.py's rule with the column-alone passes in MIOpen's place: err <= 2 err_alone + 2e-6, each
    error over the tensor's largest entry."""
    assert set(ref) == set(batched) == set(alone)
    for k, r in ref.items():
        assert r.abs().max().item() > 0, (what, k)
        e, e_alone = _err(batched[k], r), _err(alone[k], r)
        print("%s %s: batched %.3e, columns alone %.3e, ratio %.3f" % (what, k, e, e_alone, e / (2 * e_alone + 2e-6)))
        assert e <= 2 * e_alone + 2e-6, (what, k, e, e_alone)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cell", ["lstm", "gru"])
def test_cpu_layer_with_lengths_is_differentiable(cell, reverse):
    torch.manual_seed(3)
    layer = layers.Lstm(6, 16) if cell == "lstm" else layers.GruMod(6, 32)
    x = torch.randn(CPU_T, len(CPU_LENS), 6)
    dy = torch.randn(CPU_T, len(CPU_LENS), layer.rnn.hidden_size)
    got = _grads(layer, lambda v: layer(v, reverse=reverse, lengths=CPU_LENS), x, dy)
    _assert_float32_sums(got, layer, lambda m: lambda v: m(v, reverse=reverse), x, dy, CPU_LENS, CPU_LENS,
                         "%s rev %d" % (cell, reverse))
    wrapped = layers.Reverse(layer)
    if reverse:
        again = _grads(layer, lambda v: wrapped(v, lengths=CPU_LENS), x, dy)
        assert all(torch.equal(again[k], got[k]) for k in got)


def test_switch_is_off_by_default_and_the_call_then_raises(monkeypatch):
    monkeypatch.undo()
    assert layers.TRAIN_VARLEN is False
    layer = layers.Lstm(6, 16)
    with pytest.raises(RuntimeError, match="TRAIN_VARLEN"):
        layer(torch.zeros(4, 2, 6), lengths=[4, 2])
    with pytest.raises(RuntimeError, match="TRAIN_VARLEN"):
        layers.forward_varlen(_small_serial(), torch.zeros(8, 2, 1), [8, 3])


def test_cpu_forward_varlen_is_differentiable():
    torch.manual_seed(4)
    net = _small_serial()
    T, lens = 2 * CPU_T, [2 * v for v in CPU_LENS[:3]] + [9]            # 9: no multiple of the stride
    x = _padded(T, lens, 5)
    out_lens = [-(-v // 2) for v in lens]
    assert out_lens == [9, 0, 1, 5]
    dy = torch.randn(CPU_T, len(lens), 40)
    seen = {}

    def call(v):
        out, seen["lens"] = layers.forward_varlen(net, v, lens)
        return out

    got = _grads(net, call, x, dy)
    assert list(seen["lens"]) == out_lens and got["y"].shape == (CPU_T, len(lens), 40)
    _assert_float32_sums(got, net, lambda m: m, x, dy, lens, out_lens, "forward_varlen")
    # under no_grad: nothing to differentiate (nn.LSTM's inference pass on the CPU is not its training pass to the bit)
    with torch.no_grad():
        out, _ = layers.forward_varlen(net, x, lens)
    assert not out.requires_grad and (out - got["y"]).abs().max().item() <= 1e-5 * out.abs().max().item()


# ---------------------------------------------------------------------------------------------------------------------
# CPU 2: the header, the library and the binding
# ---------------------------------------------------------------------------------------------------------------------
ENTRIES = {"tk_rnn_varlen_train_workspace_bytes", "tk_lstm_forward_varlen_save_dev", "tk_lstm_backward_varlen_dev",
           "tk_gru_forward_varlen_save_dev", "tk_gru_backward_varlen_dev"}


def test_train_library_exports_exactly_what_its_header_declares():
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.VARLEN_TRAIN_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^(?:const\s+)?[a-z_0-9]+\s+\*?\s*([a-z_0-9]+)\(", hdr, flags=re.M))
    assert declared == ENTRIES
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, _lib.VARLEN_TRAIN_LIBNAME)],
                         capture_output=True, text=True, check=True).stdout
    assert {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW"} == declared
    assert set(_lib.VARLEN_TRAIN_SIGNATURES) == declared


def test_train_binding_has_the_headers_argument_types():
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    tail = [sz, sz, sz, i, i]
    assert _lib.VARLEN_TRAIN_SIGNATURES == {
        "tk_rnn_varlen_train_workspace_bytes": (sz, [i, sz, sz, i]),
        "tk_lstm_forward_varlen_save_dev": (i, [vp, vp, vp] + tail + [vp, vp, vp, vp, sz, vp, vp]),
        "tk_lstm_backward_varlen_dev": (i, [vp, vp, vp, vp, vp] + tail + [vp, vp, sz, vp, vp]),
        "tk_gru_forward_varlen_save_dev": (i, [vp, vp, vp, vp] + tail + [vp, vp, vp, vp, sz, vp, vp]),
        "tk_gru_backward_varlen_dev": (i, [vp, vp, vp, vp, vp, vp] + tail + [vp, vp, vp, sz, vp, vp]),
    }
    V, L = _lib.varlen_train_lib(), _lib.lib()
    q = V.tk_rnn_varlen_train_workspace_bytes
    # the backward's bound where the kernels run, 0 where they do not and for an unknown kind
    for n, h, cus in [(5, 256, 256), (300, 256, 256), (6, 96, 256), (300, 96, 256), (65, 256, 256), (4, 48, 256),
                      (4, 64, 0), (2049, 16, 256), (70, 32, 64)]:
        assert q(0, n, h, cus) == L.tk_lstm_workspace_bytes(n, h, cus), (n, h, cus)
        assert q(1, n, h, cus) == L.tk_gru_workspace_bytes(n, h, cus), (n, h, cus)
        assert q(2, n, h, cus) == 0 and q(-1, n, h, cus) == 0
    assert q(0, 5, 256, 256) > 0 and q(1, 6, 96, 256) > 0 and q(1, 5, 256, 256) > 0
    # argument checks, before anything is launched: NULL pointers, sizes the kernels do not cover, a short workspace
    bad, unsupported, short = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED", "WORKSPACE"))
    assert V.tk_lstm_backward_varlen_dev(None, None, None, None, None, 4, 4, 64, 0, 256, None, None, 0, None, None) == bad
    assert V.tk_gru_forward_varlen_save_dev(None, None, None, None, 4, 4, 96, 0, 256, None, None, None, None, 0, None,
                                            None) == bad
    p = ctypes.c_void_p(4096)
    assert V.tk_lstm_forward_varlen_save_dev(p, p, None, 4, 4, 48, 0, 256, p, p, p, p, 1 << 30, p, None) == unsupported
    assert V.tk_lstm_backward_varlen_dev(p, p, p, p, None, 4, 4, 64, 0, 256, p, p, 16, p, None) == short
    assert V.tk_gru_backward_varlen_dev(p, p, p, p, p, None, 4, 4, 256, 0, 256, p, p, p, 16, p, None) == short


# ---------------------------------------------------------------------------------------------------------------------
# GPU: launches at the C ABI
# ---------------------------------------------------------------------------------------------------------------------
_cus = varlen._cus
_stopped = []           # the first non-zero status word or return code of this module's own launches


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


def _nan(shape, dev):
    return torch.full(shape, float("nan"), device=dev)


def _scratch(wsb, dev):
    assert wsb > 0
    return torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)


def _dev_lens(lens, dev):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)


def _pair(kind, gx, whh, bhh, dy, lens, rev, train):
    """Forward then backward of one cell: the existing training pair (train False; lens must be None) or the pair with
    per-column lengths.  -> dict of y, gates, c (LSTM: cell; GRU: q), dgates and, for the GRU, dq."""
    T, N, HG = gx.shape
    lstm = kind == "lstm"
    ng = 4 if lstm else 3
    H, dev, cus = HG // ng, gx.device, _cus(gx.device)
    L, V = _lib.lib(), _lib.varlen_train_lib()
    if train:
        wsb = V.tk_rnn_varlen_train_workspace_bytes(0 if lstm else 1, N, H, cus)
    else:
        assert lens is None
        wsb = (L.tk_lstm_workspace_bytes if lstm else L.tk_gru_workspace_bytes)(N, H, cus)
    ld = _dev_lens(lens, dev)
    y, gates, c = _nan((T, N, H), dev), _nan((T, N, ng * H), dev), _nan((T, N, H), dev)
    dg, dq = _nan((T, N, ng * H), dev), _nan((T, N, H), dev)
    P = _lib.ptr
    dims = (T, N, H, rev, cus)

    ws, status = _scratch(wsb, dev)
    end = (P(ws), wsb, P(status), _lib.stream_ptr())
    if lstm and train:
        what, rc = "tk_lstm_forward_varlen_save_dev", V.tk_lstm_forward_varlen_save_dev(
            P(gx), P(whh), P(ld), *dims, P(y), P(gates), P(c), *end)
    elif lstm:
        what, rc = "tk_lstm_forward_dev", L.tk_lstm_forward_dev(P(gx), P(whh), *dims, P(y), P(gates), P(c), *end)
    elif train:
        what, rc = "tk_gru_forward_varlen_save_dev", V.tk_gru_forward_varlen_save_dev(
            P(gx), P(whh), P(bhh), P(ld), *dims, P(y), P(gates), P(c), *end)
    else:
        what, rc = "tk_gru_forward_dev", L.tk_gru_forward_dev(P(gx), P(whh), P(bhh), *dims, P(y), P(gates), P(c), *end)
    _finish(rc, status, what)

    ws, status = _scratch(wsb, dev)
    end = (P(ws), wsb, P(status), _lib.stream_ptr())
    if lstm and train:
        what, rc = "tk_lstm_backward_varlen_dev", V.tk_lstm_backward_varlen_dev(
            P(whh), P(gates), P(c), P(dy), P(ld), *dims, P(dg), *end)
    elif lstm:
        what, rc = "tk_lstm_backward_dev", L.tk_lstm_backward_dev(P(whh), P(gates), P(c), P(dy), *dims, P(dg), *end)
    elif train:
        what, rc = "tk_gru_backward_varlen_dev", V.tk_gru_backward_varlen_dev(
            P(whh), P(y), P(gates), P(c), P(dy), P(ld), *dims, P(dg), P(dq), *end)
    else:
        what, rc = "tk_gru_backward_dev", L.tk_gru_backward_dev(P(whh), P(y), P(gates), P(c), P(dy), *dims, P(dg),
                                                                P(dq), *end)
    _finish(rc, status, what)
    out = {"y": y, "gates": gates, "c": c, "dgates": dg}
    if not lstm:
        out["dq"] = dq
    return out


def _abi_case(kind, H, N, T, dev, seed):
    ng = 4 if kind == "lstm" else 3
    g = torch.Generator().manual_seed(seed)
    gx = torch.randn(T, N, ng * H, generator=g).to(dev)
    whh = (torch.randn(ng * H, H, generator=g) / H ** 0.5).to(dev)
    bhh = (0.3 * torch.randn(ng * H, generator=g)).to(dev)
    dy = (torch.randn(T, N, H, generator=g) / (T * N) ** 0.5).to(dev)
    return gx, whh, bhh, dy


def _inst_batch(kind, inst, dev):
    cus = _cus(dev)
    if kind == "lstm":
        n = lstm_batch(inst, cus)
        assert _lab_lstm_inst(n, inst[0], cus) == inst, (inst, n, cus)
    else:
        n = gru_batch(inst, cus)
        assert gru_rule(n, inst[0], cus) == inst, (inst, n, cus)
    return n


INSTS = [("lstm", i) for i in LSTM_INSTS] + [("gru", i) for i in GRU_INSTS]
_inst_ids = lambda v: "%s-%s" % (v[0], _ids(v[1]))


# --- 3. lengths = NULL and lengths = [T] * N: the existing training pair, bit for bit --------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("case", INSTS, ids=_inst_ids)
def test_full_lengths_are_the_existing_training_pair_bit_for_bit(gpu_device, case, rev):
    kind, inst = case
    H, n = inst[0], _inst_batch(kind, inst, gpu_device)
    for T in STEPS + ([21] if H == 256 else []):
        gx, whh, bhh, dy = _abi_case(kind, H, n, T, gpu_device, 500 + H + 10 * T + rev)
        want = _pair(kind, gx, whh, bhh, dy, None, rev, train=False)
        for lens in (None, [T] * n):
            got = _pair(kind, gx, whh, bhh, dy, lens, rev, train=True)
            assert set(got) == set(want)
            for k in want:
                assert bool(torch.isfinite(want[k]).all()), (case, T, k)
                assert torch.equal(got[k], want[k]), (case, T, rev, "NULL" if lens is None else "[T] * N", k,
                                                      (got[k] - want[k]).abs().max().item())


# --- 4. every column against the column run alone --------------------------------------------------------------------
def _check_columns_alone(kind, gx, whh, bhh, dy, lens, rev, columns, exact, what):
    """The launch with lengths, NaN in gx and dy beyond them, against the existing pair on each of `columns` alone."""
    T, N, _ = gx.shape
    dev = gx.device
    beyond = torch.arange(T, device=dev)[:, None] >= torch.tensor(lens, device=dev)[None, :]
    gxp, dyp = gx.clone(), dy.clone()
    gxp[beyond], dyp[beyond] = float("nan"), float("nan")
    assert bool(torch.isnan(gxp).any()) and bool(torch.isnan(dyp).any())
    got = _pair(kind, gxp, whh, bhh, dyp, lens, rev, train=True)
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (what, k, "a non-finite value")
        assert not v[beyond].any(), (what, k, "rows at and beyond the length are not exactly 0")
    for n in columns:
        ln = lens[n]
        if ln == 0:
            continue
        alone = _pair(kind, gx[:ln, n:n + 1].contiguous(), whh, bhh, dy[:ln, n:n + 1].contiguous(), None, rev,
                      train=False)
        for k in ("dgates", "dq", "y", "gates", "c"):
            if k not in got:
                continue
            a, b = got[k][:ln, n], alone[k][:, 0]
            if exact:
                assert torch.equal(a, b), (what, n, k, (a - b).abs().max().item())
            else:
                err, bound = (a - b).abs().max().item(), 1e-5 * a.abs().max().item()
                print("%s column %d %s: max|a - b| %.3g, bound %.3g" % (what, n, k, err, bound))
                assert err <= bound, (what, n, k, err, bound)


def _sample(n):
    """Every column of a small batch; of a large one 16: the first and last 7 (every length of lengths_for's pattern,
    at both ends and so in a ragged last workgroup) and two in the middle."""
    if n <= 16:
        return list(range(n))
    return sorted(set(range(7)) | {n // 2, n // 2 + 1} | set(range(n - 7, n)))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("case", INSTS, ids=_inst_ids)
def test_columns_equal_the_column_run_alone(gpu_device, case, rev):
    kind, inst = case
    H, T, n = inst[0], 7, _inst_batch(kind, inst, gpu_device)
    lens = lengths_for(n, T)
    assert {0, 1, T - 1, T} <= set(lens)
    if kind == "lstm":
        exact = varlen._lstm_same_geometry(n, H, _cus(gpu_device))
    else:
        exact = inst[1] == 1 or H == 256
    gx, whh, bhh, dy = _abi_case(kind, H, n, T, gpu_device, 600 + H + rev)
    cols = _sample(n)
    assert {lens[c] for c in cols} == set(lens)
    _check_columns_alone(kind, gx, whh, bhh, dy, lens, rev, cols, exact, "%s rev %d" % (_inst_ids(case), rev))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
def test_gru_two_columns_per_workgroup_against_the_column_alone(gpu_device, rev):
    """tests/test_rnn_varlen.py::test_gru_two_columns_per_workgroup's launch (more columns than CUs, lengths n % 9 at
    T 8, its sample of 16 columns) through the training pair: not the same (U, C), the rounding-level rule."""
    H, T = 96, 8
    N = _cus(gpu_device) + 44
    assert gru_rule(N, H, _cus(gpu_device)) == (H, 2)
    lens = [n % 9 for n in range(N)]
    sample = sorted({0, 1, 7, 8, 16, 17, 26, 35, 100, 101, N // 2, N // 2 + 1, N - 4, N - 3, N - 2, N - 1})
    assert len(sample) == 16
    gx, whh, bhh, dy = _abi_case("gru", H, N, T, gpu_device, 700 + rev)
    _check_columns_alone("gru", gx, whh, bhh, dy, lens, rev, sample, False, "gru C 2 rev %d" % rev)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the layers
# ---------------------------------------------------------------------------------------------------------------------
def _layer_lengths(N, T):
    """0, 1, T - 1 and T among them, for any N >= 4."""
    pat = (T, 0, 1, T - 1, T // 2, T, 3)
    return [min(pat[n % 7], T) for n in range(N)]


def _make_layer(cell, I, H):
    return layers.Lstm(I, H) if cell == "lstm" else layers.GruMod(I, H)


@functools.lru_cache(maxsize=None)
def _layer_case(cell, T, N, H, I, reverse):
    """The layer at its own initialisation, x (random in the padding too: finite is all the rule asks), dy, the lengths
    and the float64 reference: every column alone on the CPU (computed once, shared, never written)."""
    torch.manual_seed(9000 + T + N + H + I + int(reverse))
    layer = _make_layer(cell, I, H)
    x, dy = torch.randn(T, N, I), torch.randn(T, N, H) / (T * N) ** 0.5
    lens = _layer_lengths(N, T)
    l64 = copy.deepcopy(layer).double()
    ref = _column_sums(l64, lambda v: l64(v, reverse=reverse), x.double(), dy.double(), lens, lens)
    return layer, x, dy, lens, ref


LAYER_SHAPES = [("lstm", 37, 5, 64, 16), ("lstm", 20, 9, 256, 256), ("lstm", 25, 70, 32, 20),
                ("gru", 41, 5, 96, 16), ("gru", 23, 6, 256, 64)]


# --- 5. the layer against float64 ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cell,T,N,H,I,wgrad", [s + (w,) for s in LAYER_SHAPES for w in ((True, False) if s[0] == "lstm"
                                                                                         else (True,))])
def test_layer_with_lengths_matches_float64(gpu_device, cell, T, N, H, I, wgrad, reverse):
    """wgrad: layers.USE_HIP_LSTM_WGRAD, the LSTM's switch (on both sides of the comparison)."""
    layer, x, dy, lens, ref = _layer_case(cell, T, N, H, I, reverse)
    dev = gpu_device
    layer = copy.deepcopy(layer).to(dev)
    xg, dyg = x.to(dev), dy.to(dev)
    assert layers.hip_rnn_varlen_train_workspace_bytes(layer.rnn, xg) > 0
    old = layers.USE_HIP_LSTM_WGRAD
    before = dict(layers.rnn_varlen_calls)
    try:
        layers.USE_HIP_LSTM_WGRAD = wgrad
        batched = _grads(layer, lambda v: layer(v, reverse=reverse, lengths=lens), xg, dyg)
        assert layers.rnn_varlen_calls == dict(before, saved=before["saved"] + 1)
        alone = _column_sums(layer, lambda v: layer(v, reverse=reverse), xg, dyg, lens, lens)
    finally:
        layers.USE_HIP_LSTM_WGRAD = old
    assert layers.rnn_varlen_calls["saved"] == before["saved"] + 1, "a column alone took the launch with lengths"
    beyond = torch.arange(T)[:, None] >= torch.as_tensor(lens)[None, :]
    assert not batched["y"].cpu()[beyond].any() and not batched["x"].cpu()[beyond].any()
    _compare_with_columns_alone(ref, batched, alone, "%s T %d N %d H %d I %d rev %d wgrad %d"
                                % (cell, T, N, H, I, reverse, wgrad))


# --- 6. the padding is inert -----------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cell,T,N,H,I", [("lstm", 20, 9, 256, 256), ("lstm", 37, 5, 64, 16), ("gru", 41, 5, 96, 16),
                                          ("gru", 23, 6, 256, 64)])
def test_padding_of_x_is_inert(gpu_device, cell, T, N, H, I, reverse):
    layer, x, dy, lens, _ = _layer_case(cell, T, N, H, I, reverse)
    layer = copy.deepcopy(layer).to(gpu_device)
    beyond = torch.arange(T)[:, None] >= torch.as_tensor(lens)[None, :]
    assert int(beyond.sum()) > 0
    got = []
    for fill in (0.0, 1e3):
        xp = x.clone()
        xp[beyond] = fill
        got.append(_grads(layer, lambda v: layer(v, reverse=reverse, lengths=lens), xp.to(gpu_device),
                          dy.to(gpu_device)))
    a, b = got
    assert set(a) == set(b) and len(a) >= 5
    for k in a:
        assert bool(torch.isfinite(a[k]).all()) and a[k].abs().max().item() > 0, k
        assert torch.equal(a[k], b[k]), (cell, reverse, k, (a[k] - b[k]).abs().max().item())
    assert not b["x"].cpu()[beyond].any() and not b["y"].cpu()[beyond].any()


# --- 7. forward_varlen under grad mode -------------------------------------------------------------------------------
def _network(name):
    torch.manual_seed(12)
    if name == "small":
        return _small_serial(), 2, [40, 0, 1, 39, 21, 40, 3]
    return models.mLstm_flipflop(size=64, stride=5), 5, [60, 0, 1, 59, 33, 60, 3]


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["small", "mLstm"])
def test_forward_varlen_gradients_match_the_columns_alone(gpu_device, name):
    net, stride, lens = _network(name)
    T, N, dev = max(lens), len(lens), gpu_device
    out_lens = [-(-v // stride) for v in lens]
    x = _padded(T, lens, 13)
    dy = torch.randn(max(out_lens), N, 40, generator=torch.Generator().manual_seed(14)) / (T * N) ** 0.5
    n64 = copy.deepcopy(net).double()
    ref = _column_sums(n64, n64, x.double(), dy.double(), lens, out_lens)
    net = net.to(dev)
    xg, dyg = x.to(dev), dy.to(dev)
    nrnn = sum(isinstance(m, (layers.Lstm, layers.GruMod)) for m in net.modules())
    ngru = sum(isinstance(m, layers.GruMod) for m in net.modules())

    before, gbefore = dict(layers.rnn_varlen_calls), dict(layers.gru_forward_calls)
    batched = _grads(net, lambda v: layers.forward_varlen(net, v, lens)[0], xg, dyg)
    assert layers.rnn_varlen_calls == dict(before, saved=before["saved"] + nrnn), "not the launches that save"
    assert layers.gru_forward_calls == dict(gbefore, saved=gbefore["saved"] + ngru)
    alone = _column_sums(net, net, xg, dyg, lens, out_lens)
    beyond = torch.arange(max(out_lens))[:, None] >= torch.as_tensor(out_lens)[None, :]
    assert not batched["y"].cpu()[beyond].any()
    assert not batched["x"].cpu()[torch.arange(T)[:, None] >= torch.as_tensor(lens)[None, :]].any()
    _compare_with_columns_alone(ref, batched, alone, "forward_varlen %s" % name)

    # under no_grad: the launches that save nothing, as before, and the same rows
    before, gbefore = dict(layers.rnn_varlen_calls), dict(layers.gru_forward_calls)
    with torch.no_grad():
        out, got_lens = layers.forward_varlen(net, xg, lens)
        again, _ = layers.forward_varlen(net, xg, lens)
    assert layers.rnn_varlen_calls == dict(before, inference=before["inference"] + 2 * nrnn), "the saving path was taken"
    assert layers.gru_forward_calls == gbefore
    assert list(got_lens) == out_lens and not out.requires_grad
    assert torch.equal(out, again)
    assert (out - batched["y"]).abs().max().item() <= 1e-5 * out.abs().max().item()


# --- 8. a captured forward + backward replays bit-identically --------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("cell,T,N,H,I", [("lstm", 30, 9, 64, 32), ("gru", 30, 9, 256, 32)])
def test_captured_forward_and_backward_replay_bit_identical(gpu_device, cell, T, N, H, I):
    torch.manual_seed(7)
    dev = gpu_device
    layer = layers.Reverse(_make_layer(cell, I, H)).to(dev)
    params = [p for p in layer.parameters() if p.requires_grad]
    x = torch.randn(T, N, I, device=dev).requires_grad_(True)
    dy = torch.randn(T, N, H, device=dev)
    lens = torch.tensor(_layer_lengths(N, T), dtype=torch.int32, device=dev)

    def step():
        y = layer(x, lengths=lens)
        return (y,) + torch.autograd.grad((y * dy).sum(), [x] + params)

    strict = _lib.is_strict()
    _lib.set_strict(False)
    try:
        eager = [v.detach().clone() for v in step()]
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            step()
        torch.cuda.current_stream().wait_stream(side)
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            out = step()
        for _ in range(3):
            for v in out:
                v.detach().fill_(float("nan"))
            g.replay()
            torch.cuda.synchronize()
            for v, e in zip(out, eager):
                assert torch.equal(v.detach(), e)
        _lib.raise_if_nonfinite()
    finally:
        _lib.set_strict(strict)


# --- 9. one Function per cell: full lengths are the call without lengths, bit for bit --------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("cell,H", [("lstm", 128), ("lstm", 32), ("gru", 256), ("gru", 32)])
def test_full_lengths_are_the_call_without_lengths(gpu_device, cell, H, reverse):
    """`LstmRecurrence` / `GruRecurrence` take the lengths as an argument: layer(x, lengths=[T] * N) and layer(x) differ
    in the library, the entry points, the workspace tag and the counters, and in nothing that is computed.  The kernels
    with lengths = [T] * N are the kernels without, bit for bit (pinned at the C ABI above); the GEMMs and the
    weight-gradient kernel are the same calls on the same tensors.  So y, dx and every parameter gradient are
    torch.equal; a second run of the call without lengths, asserted equal to the first here, shows that the path is
    reproducible run to run, which is what makes torch.equal the right comparison.  Sizes: 128 is two LSTM workgroups
    that hand h over, 256 the GRU's four members, 32 one workgroup."""
    T, N, I, dev = 5, 3, 8, gpu_device
    torch.manual_seed(77)
    layer = _make_layer(cell, I, H).to(dev)
    x, w = torch.randn(T, N, I, device=dev), torch.randn(T, N, H, device=dev)
    gru = int(cell == "gru")

    before, gbefore = dict(layers.rnn_varlen_calls), dict(layers.gru_forward_calls)
    plain = _grads(layer, lambda v: layer(v, reverse=reverse), x, w)
    again = _grads(layer, lambda v: layer(v, reverse=reverse), x, w)
    assert layers.rnn_varlen_calls == before
    assert layers.gru_forward_calls == dict(gbefore, saved=gbefore["saved"] + 2 * gru)
    assert set(plain) == set(again) and len(plain) == 5           # y, x, weight_ih, weight_hh, bias_ih
    for k in plain:
        assert bool(torch.isfinite(plain[k]).all()) and plain[k].abs().max().item() > 0, k
        assert torch.equal(plain[k], again[k]), ("run to run", k, (plain[k] - again[k]).abs().max().item())

    before, gbefore = dict(layers.rnn_varlen_calls), dict(layers.gru_forward_calls)
    full = _grads(layer, lambda v: layer(v, reverse=reverse, lengths=[T] * N), x, w)
    assert layers.rnn_varlen_calls == dict(before, saved=before["saved"] + 1)
    assert layers.gru_forward_calls == dict(gbefore, saved=gbefore["saved"] + gru)
    assert set(full) == set(plain)
    for k in plain:
        assert torch.equal(full[k], plain[k]), (cell, H, reverse, k, (full[k] - plain[k]).abs().max().item())

    # nothing to differentiate: the launch with lengths that saves nothing, counted as such and nowhere else
    before, gbefore = dict(layers.rnn_varlen_calls), dict(layers.gru_forward_calls)
    with torch.no_grad():
        y = layer(x, reverse=reverse, lengths=[T] * N)
    assert layers.rnn_varlen_calls == dict(before, inference=before["inference"] + 1)
    assert layers.gru_forward_calls == gbefore
    assert not y.requires_grad and y.shape == plain["y"].shape
