"""include/taiyaki_amd_lstm_large.h on the host: the header, the library and the binding, the geometry's queries restated,
the argument checks in front of a launch (fake pointers, never dereferenced: every check under test returns before any
HIP call), and what stays as it was (the other libraries' queries at size 512, CPU tensors)."""
import ctypes
import os
import re
import subprocess

import pytest
import torch

from taiyaki_amd import _lib, layers

H = 512
UNITS, MEMBERS = 32, 16                 # hidden units per workgroup; workgroups of a group
COLUMNS = (4, 8)                        # batch columns per group, in the order the rule tries them
ENTRIES = {"tk_lstm_large_supported", "tk_lstm_large_slab", "tk_lstm_large_workspace_bytes",
           "tk_lstm_large_forward_dev", "tk_lstm_large_backward_dev"}
LAB_ENTRIES = {"tk_lab_lstm_large_cols", "tk_lab_lstm_large_geometry"}
BAD_ARG, UNSUPPORTED, WORKSPACE = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED", "WORKSPACE"))


def rule(n, cus, columns=COLUMNS):
    """(C, groups) of the launch that admits a batch of n on `cus` CUs, or None: the first C of `columns` whose
    ceil(n / C) groups of 16 workgroups fit one workgroup per CU."""
    if n <= 0 or cus <= 0:
        return None
    for c in columns:
        groups = -(-n // c)
        if groups * MEMBERS <= cus:
            return c, groups
    return None


def bound(cus, columns=COLUMNS):
    """The widest batch one launch admits."""
    return max(columns) * (cus // MEMBERS)


def granule_bytes(c, groups, backward):
    return 2 * groups * (MEMBERS if backward else 1) * c * H * 8


def _exported(libname):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                         capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def _lab():
    return _lib.use_lab(True) and _lib.lstm_large_lib()


def test_header_binding_and_exports_name_the_same_entries():
    assert set(_lib.LSTM_LARGE_SIGNATURES) == ENTRIES and set(_lib.LSTM_LARGE_LAB_SIGNATURES) == LAB_ENTRIES
    assert _exported(_lib.LSTM_LARGE_LIBNAME) == ENTRIES
    assert _exported(_lib.LSTM_LARGE_LAB_LIBNAME) == ENTRIES | LAB_ENTRIES
    L = _lib.lstm_large_lib()                           # resolves every symbol
    assert not hasattr(L, "tk_lab_lstm_large_cols")
    sz, i, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    sigs = _lib.LSTM_LARGE_SIGNATURES
    assert sigs["tk_lstm_large_supported"] == (i, [sz])
    assert sigs["tk_lstm_large_slab"] == sigs["tk_lstm_large_workspace_bytes"] == (sz, [sz, sz, i])
    assert sigs["tk_lstm_large_forward_dev"] == (i, [vp, vp, vp, sz, sz, sz, i, i, vp, vp, vp, vp, sz, vp, vp])
    assert sigs["tk_lstm_large_backward_dev"] == (i, [vp, vp, vp, vp, vp, sz, sz, sz, i, i, vp, vp, sz, vp, vp])
    # the version script takes the prefix, the header the names: the lab hooks are declared under TK_LAB only
    header = open(_lib.LSTM_LARGE_HEADER).read()
    lab = re.search(r"#ifdef TK_LAB\n(.*?)#endif", header, re.S).group(1)
    assert all(name in lab for name in LAB_ENTRIES) and "tk_lab_" not in header.replace(lab, "")
    try:
        lab_lib = _lab()
        assert lab_lib is not L and all(hasattr(lab_lib, name) for name in LAB_ENTRIES)
    finally:
        _lib.use_lab(False)
    assert _lib.lstm_large_lib() is L


def test_supported_at_512_alone():
    L = _lib.lstm_large_lib()
    assert L.tk_lstm_large_supported(H) == 1
    for h in (0, 96, 256, 384, 511, 768, 1024):
        assert L.tk_lstm_large_supported(h) == 0, h
        assert L.tk_lstm_large_slab(5, h, 256) == 0 and L.tk_lstm_large_workspace_bytes(5, h, 256) == 0, h


@pytest.mark.parametrize("cus", [256, 64])
def test_queries_restate_the_rule(cus):
    """Every N from 1 to one past the widest launch: the slab, the workspace (the backward's granules at the widest
    slab: 2 x groups x 16 x C x 512 x 8) and the lab geometry's eight numbers, the grid never above the CUs."""
    L = _lib.lstm_large_lib()
    S = bound(cus)
    assert S == {256: 128, 64: 32}[cus] and rule(S, cus) is not None and rule(S + 1, cus) is None
    assert rule(bound(cus, COLUMNS[:1]), cus)[0] == 4 and rule(bound(cus, COLUMNS[:1]) + 1, cus)[0] == COLUMNS[-1]
    out = (ctypes.c_size_t * 8)()
    try:
        lab = _lab()
        lab.tk_lab_lstm_large_cols(0)
        for n in range(1, S + 2):
            slab = min(n, S)
            c, groups = rule(slab, cus)
            assert L.tk_lstm_large_slab(n, H, cus) == slab, (n, cus)
            assert L.tk_lstm_large_workspace_bytes(n, H, cus) == 2 * groups * 16 * c * 512 * 8, (n, cus)
            assert lab.tk_lab_lstm_large_geometry(n, H, cus, out) == (1 if n <= S else 0), (n, cus)
            if n <= S:
                grid = groups * MEMBERS
                assert grid <= cus
                assert list(out) == [c, groups, UNITS, c, groups, grid, granule_bytes(c, groups, False),
                                     granule_bytes(c, groups, True)], (n, cus, list(out))
        assert L.tk_lstm_large_slab(3 * S + 5, H, cus) == S
        assert L.tk_lstm_large_workspace_bytes(3 * S + 5, H, cus) == L.tk_lstm_large_workspace_bytes(S, H, cus)
    finally:
        _lib.use_lab(False)
    # nothing runs: no batch, no CUs, fewer CUs than one group
    for n, c in ((0, cus), (5, 0), (5, -1), (5, 15)):
        assert L.tk_lstm_large_slab(n, H, c) == 0 and L.tk_lstm_large_workspace_bytes(n, H, c) == 0, (n, c)
    assert L.tk_lstm_large_slab(5, H, 16) == 5


def test_lab_hook_forces_the_columns():
    out = (ctypes.c_size_t * 8)()
    try:
        lab = _lab()
        for forced in COLUMNS:
            lab.tk_lab_lstm_large_cols(forced)
            S = bound(256, (forced,))
            assert lab.tk_lstm_large_slab(1000, H, 256) == S
            assert lab.tk_lab_lstm_large_geometry(5, H, 256, out) == 1 and out[3] == forced and out[4] == -(-5 // forced)
            assert lab.tk_lab_lstm_large_geometry(S + 1, H, 256, out) == 0
        lab.tk_lab_lstm_large_cols(0)
        assert lab.tk_lab_lstm_large_geometry(5, H, 256, out) == 1 and out[3] == 4
        assert lab.tk_lab_lstm_large_geometry(5, 256, 256, out) == 0
    finally:
        lab.tk_lab_lstm_large_cols(0)
        _lib.use_lab(False)


def test_the_other_libraries_still_answer_0_at_512():
    kind = _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"]
    for n in (1, 6, 128, 300):
        assert _lib.lib().tk_lstm_workspace_bytes(n, H, 256) == 0
        assert _lib.varlen_lib().tk_rnn_varlen_workspace_bytes(kind, n, H, 256) == 0
        assert _lib.varlen_train_lib().tk_rnn_varlen_train_workspace_bytes(kind, n, H, 256) == 0
        assert _lib.rnn_wide_lib().tk_rnn_wide_workspace_bytes(kind, n, H, 256) == 0
        assert _lib.rnn_wide_lib().tk_rnn_wide_slab(kind, n, H, 256) == 0
    assert _lib.lstm_local_lib().tk_lstm_local_supported(H) == 0


FWD = "gx w_hh lengths nblk nbatch size reverse cu_count y gates cell workspace workspace_bytes status stream".split()
BWD = ("w_hh gates cell dy lengths nblk nbatch size reverse cu_count dgates workspace workspace_bytes status "
       "stream").split()
SCALARS = ("nblk", "nbatch", "size", "reverse", "cu_count", "workspace_bytes", "stream")


class Entry:
    """One entry with fake pointers everywhere (4096: non-NULL and 16-byte aligned), nblk = 4 and workspace_bytes = 0;
    `over` replaces arguments by name.  It refuses to make a call that could launch: one whose size has a plan, with
    nblk > 0 and a workspace at or above the launch's need."""

    def __init__(self, backward, nbatch, cus):
        L = _lib.lstm_large_lib()
        self.fn = L.tk_lstm_large_backward_dev if backward else L.tk_lstm_large_forward_dev
        self.names, self.nbatch, self.cus = BWD if backward else FWD, nbatch, cus
        self.optional = ("lengths",) if backward else ("lengths", "gates", "cell")
        c, groups = rule(min(nbatch, bound(cus)), cus)
        self.need = granule_bytes(c, groups, backward)          # of the first slab, the widest
        self.query = L.tk_lstm_large_workspace_bytes(nbatch, H, cus)
        self.pointers = [n for n in self.names if n not in SCALARS]

    def __call__(self, **over):
        args = dict(nblk=4, nbatch=self.nbatch, size=H, reverse=0, cu_count=self.cus, workspace_bytes=0, stream=None)
        args.update({n: ctypes.c_void_p(4096) for n in self.pointers})
        assert set(over) <= set(args), over
        args.update(over)
        assert args["nblk"] == 0 or args["workspace_bytes"] < self.need or args["size"] != H, "this call could launch"
        return self.fn(*[args[n] for n in self.names])


@pytest.mark.parametrize("backward", [False, True], ids=["forward", "backward"])
@pytest.mark.parametrize("nbatch,cus", [(5, 256), (64, 256), (65, 256), (300, 256), (40, 64)])
def test_entry_checks(backward, nbatch, cus):
    """tests/test_rnn_entry_checks.py's sequence at the two new entries, at one launch of either column count and at
    batches that run as slabs."""
    e = Entry(backward, nbatch, cus)
    assert 0 < e.need <= e.query and e.need % 16 == 0
    assert (e.need == e.query) == backward
    # required pointers, one at a time; the workspace's alignment (the pointer check is the first: it answers whatever
    # workspace_bytes says)
    for p in e.pointers:
        if p not in e.optional:
            assert e(**{p: None}) == BAD_ARG, p
    assert e(workspace=ctypes.c_void_p(4100)) == BAD_ARG
    # optional pointers: the call passes the pointer check and stops at the workspace's size
    assert e() == WORKSPACE
    assert e(lengths=None) == WORKSPACE
    if backward:
        assert e(gates=None) == BAD_ARG and e(cell=None) == BAD_ARG
    else:
        assert e(gates=None, cell=None) == WORKSPACE and e(gates=None, cell=None, lengths=None) == WORKSPACE
        # one of the two saved tensors NULL alone, whatever else the call holds
        assert e(gates=None) == BAD_ARG and e(cell=None) == BAD_ARG
        assert e(gates=None, workspace_bytes=e.need - 1) == BAD_ARG and e(cell=None, size=256) == BAD_ARG
    # no plan, whatever the workspace: asked before the workspace
    for size in (256, 384, 96, 1024):
        assert e(size=size, workspace_bytes=1 << 40) == UNSUPPORTED and e(size=size) == UNSUPPORTED, size
    assert e(nbatch=0) == UNSUPPORTED and e(cu_count=0) == UNSUPPORTED and e(cu_count=15) == UNSUPPORTED
    # the last byte of the launch's need
    assert e(workspace_bytes=e.need - 1) == WORKSPACE
    # nblk = 0: nothing to do, nothing touched; the workspace is still checked
    assert e(nblk=0, workspace_bytes=e.query) == 0
    assert e(nblk=0, workspace_bytes=e.need) == 0
    assert e(nblk=0, workspace_bytes=e.need - 1) == WORKSPACE
    assert e(nblk=0, size=256, workspace_bytes=e.query) == UNSUPPORTED
    # nblk or nbatch beyond int32: with the pointers', in front of the plan and the workspace
    assert e(nblk=2 ** 31) == BAD_ARG and e(nbatch=2 ** 31) == BAD_ARG and e(nblk=2 ** 31, size=256) == BAD_ARG
    assert e(nblk=2 ** 31 - 1) == WORKSPACE


def test_cpu_tensors_and_the_switch_take_nn_lstm(monkeypatch):
    assert layers.USE_HIP_LSTM_LARGE is True and layers.lstm_large_calls.keys() == {"saved", "inference"}
    torch.manual_seed(0)
    lstm = layers.Lstm(12, H)
    x = torch.randn(5, 3, 12)
    before = dict(layers.lstm_large_calls)
    assert layers.hip_lstm_large_workspace_bytes(lstm.rnn, x) == 0 and layers.hip_lstm_workspace_bytes(lstm.rnn, x) == 0
    assert layers.hip_lstm_large_workspace_bytes(layers.GruMod(12, H).rnn, x) == 0
    assert torch.equal(lstm(x), lstm.rnn(x)[0])
    assert torch.equal(layers.Reverse(lstm)(x), torch.flip(lstm.rnn(torch.flip(x, (0,)))[0], (0,)))
    with torch.no_grad():
        y = lstm(x, lengths=[5, 2, 0])
        assert torch.equal(y[:2, 1:2], lstm.rnn(x[:2, 1:2])[0]) and not y[2:, 1].any() and not y[:, 2].any()
    assert layers.lstm_large_calls == before
    assert ("large", True) in layers._RNN_LAUNCHES and ("large", False) in layers._RNN_LAUNCHES
    for save in (True, False):
        libname, fwd, bwd, _ = layers._RNN_LAUNCHES["large", save]
        assert getattr(_lib, libname) is _lib.lstm_large_lib and fwd % "lstm" in ENTRIES
        assert (bwd % "lstm" in ENTRIES) if save else bwd is None
