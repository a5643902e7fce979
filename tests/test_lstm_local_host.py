"""include/taiyaki_amd_lstm_local.h on the host: the header, the library and the binding, the plan's query, the argument
checks in front of a launch, and what stays as it was (the existing queries at size 96, CPU tensors)."""
import ctypes
import os
import re
import subprocess

import torch

from taiyaki_amd import _lib, layers

ENTRIES = {"tk_lstm_local_supported", "tk_lstm_local_columns", "tk_lstm_local_forward_dev", "tk_lstm_local_backward_dev"}
LAB_ENTRIES = {"tk_lab_lstm_local_cols"}


def _exported(libname):
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, libname)], check=True,
                         capture_output=True, text=True).stdout
    return {line.split()[-1] for line in out.splitlines() if line.strip()}


def test_header_binding_and_exports_name_the_same_entries():
    assert set(_lib.LSTM_LOCAL_SIGNATURES) == ENTRIES and set(_lib.LSTM_LOCAL_LAB_SIGNATURES) == LAB_ENTRIES
    assert _exported(_lib.LSTM_LOCAL_LIBNAME) == ENTRIES
    assert _exported(_lib.LSTM_LOCAL_LAB_LIBNAME) == ENTRIES | LAB_ENTRIES
    L = _lib.lstm_local_lib()                           # resolves every symbol
    assert not hasattr(L, "tk_lab_lstm_local_cols")
    sz, i, vp = ctypes.c_size_t, ctypes.c_int, ctypes.c_void_p
    assert _lib.LSTM_LOCAL_SIGNATURES["tk_lstm_local_forward_dev"] == (i, [vp, vp, vp, sz, sz, sz, i, i, vp, vp, vp, vp])
    assert _lib.LSTM_LOCAL_SIGNATURES["tk_lstm_local_backward_dev"] == (i, [vp, vp, vp, vp, vp, sz, sz, sz, i, i, vp, vp])
    # the version script takes the prefix, the header the names: the lab hook is declared under TK_LAB only
    header = open(_lib.LSTM_LOCAL_HEADER).read()
    lab = re.search(r"#ifdef TK_LAB\n(.*?)#endif", header, re.S).group(1)
    assert "tk_lab_lstm_local_cols" in lab and "tk_lab_" not in header.replace(lab, "")
    try:
        lab_lib = _lib.use_lab(True) and _lib.lstm_local_lib()
        assert lab_lib is not L and hasattr(lab_lib, "tk_lab_lstm_local_cols")
    finally:
        _lib.use_lab(False)
    assert _lib.lstm_local_lib() is L


def test_supported_sizes():
    L = _lib.lstm_local_lib()
    assert L.tk_lstm_local_supported(96) == 1
    for h in (0, 16, 48, 64, 95, 97, 128, 192, 256, 384, 512):
        assert L.tk_lstm_local_supported(h) == 0, h


def test_columns_follow_the_documented_rule():
    L = _lib.lstm_local_lib()
    q = L.tk_lstm_local_columns
    assert q(0, 96, 256) == 0 and q(5, 96, 0) == 0 and q(5, 96, -1) == 0 and q(5, 256, 256) == 0
    for cus in (256, 64):
        for n in range(1, 601):
            assert q(n, 96, cus) == (1 if n <= cus else 2), (n, cus)
    try:
        lab = _lib.use_lab(True) and _lib.lstm_local_lib()
        for forced, want in ((1, 1), (2, 2), (0, 1)):
            lab.tk_lab_lstm_local_cols(forced)
            assert lab.tk_lstm_local_columns(5, 96, 256) == want and lab.tk_lstm_local_columns(5, 256, 256) == 0
    finally:
        lab.tk_lab_lstm_local_cols(0)
        _lib.use_lab(False)


def test_entries_check_their_arguments_before_anything_is_launched():
    L = _lib.lstm_local_lib()
    bad, unsupported = (_lib.DEFINES["TK_ERR_" + k] for k in ("BAD_ARG", "UNSUPPORTED"))
    p, odd = ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    fwd, bwd = L.tk_lstm_local_forward_dev, L.tk_lstm_local_backward_dev
    # a required pointer NULL or misaligned
    assert fwd(None, p, None, 4, 3, 96, 0, 256, p, p, p, None) == bad
    assert fwd(p, None, None, 4, 3, 96, 0, 256, p, p, p, None) == bad
    assert fwd(p, p, None, 4, 3, 96, 0, 256, None, p, p, None) == bad
    assert fwd(odd, p, None, 4, 3, 96, 0, 256, p, p, p, None) == bad
    assert bwd(p, p, p, None, None, 4, 3, 96, 0, 256, p, None) == bad
    assert bwd(p, p, p, p, None, 4, 3, 96, 0, 256, None, None) == bad
    # one of the two saved tensors NULL alone
    assert fwd(p, p, None, 4, 3, 96, 0, 256, p, p, None, None) == bad
    assert fwd(p, p, None, 4, 3, 96, 0, 256, p, None, p, None) == bad
    # nblk or nbatch beyond int32, in front of the size
    assert fwd(p, p, None, 1 << 31, 3, 256, 0, 256, p, p, p, None) == bad
    assert bwd(p, p, p, p, None, 4, 1 << 31, 96, 0, 256, p, None) == bad
    # a size the kernels do not cover, no batch, no CUs: behind the pointer checks, in front of nblk = 0
    assert fwd(p, p, None, 4, 3, 256, 0, 256, p, p, p, None) == unsupported
    assert fwd(p, p, None, 4, 0, 96, 0, 256, p, p, p, None) == unsupported
    assert fwd(p, p, None, 0, 3, 96, 0, 0, p, None, None, None) == unsupported
    assert bwd(p, p, p, p, None, 4, 3, 512, 0, 256, p, None) == unsupported
    assert bwd(p, p, p, p, None, 0, 0, 96, 0, 256, p, None) == unsupported
    # nothing to do at nblk = 0, behind the checks
    assert fwd(p, p, None, 0, 3, 96, 0, 256, p, p, p, None) == 0
    assert fwd(p, p, p, 0, 3, 96, 1, 256, p, None, None, None) == 0
    assert bwd(p, p, p, p, p, 0, 300, 96, 0, 256, p, None) == 0


def test_existing_queries_still_refuse_size_96():
    kind = _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"]
    for n in (1, 6, 128, 300):
        assert _lib.lib().tk_lstm_workspace_bytes(n, 96, 256) == 0
        assert _lib.varlen_lib().tk_rnn_varlen_workspace_bytes(kind, n, 96, 256) == 0
        assert _lib.varlen_train_lib().tk_rnn_varlen_train_workspace_bytes(kind, n, 96, 256) == 0
        assert _lib.rnn_wide_lib().tk_rnn_wide_workspace_bytes(kind, n, 96, 256) == 0


def test_cpu_tensors_take_nn_lstm_bit_for_bit():
    assert layers.USE_HIP_LSTM_LOCAL is True and layers.lstm_local_calls.keys() == {"saved", "inference"}
    torch.manual_seed(0)
    lstm = layers.Lstm(12, 96)
    x = torch.randn(9, 3, 12)
    before = dict(layers.lstm_local_calls)
    assert not layers.hip_lstm_local_takes(lstm.rnn, x) and layers.hip_lstm_workspace_bytes(lstm.rnn, x) == 0
    assert torch.equal(lstm(x), lstm.rnn(x)[0])
    assert torch.equal(layers.Reverse(lstm)(x), torch.flip(lstm.rnn(torch.flip(x, (0,)))[0], (0,)))
    with torch.no_grad():
        y = lstm(x, lengths=[9, 4, 0])
        assert torch.equal(y[:4, 1:2], lstm.rnn(x[:4, 1:2])[0]) and not y[4:, 1].any() and not y[:, 2].any()
    assert layers.lstm_local_calls == before
