"""The decode operators with a length per column (include/taiyaki_amd_decode_varlen.h; `decode.flipflop_viterbi_path` and
`decode.flipflop_make_trans` with `lengths`).

CPU: the header is the ABI, the binding has its argument types, lengths are checked before anything is launched, and the
float64 forward-backward restated here (the reference of the GPU tests) agrees with the oracle at full-length columns.
GPU: every column against the existing fixed-length operator on the column alone -- the Viterbi bit for bit, the
posterior under the project's rule against float64 -- and the gather against numpy, bit for bit.  Every alphabet size the
library is built for (nbase 1 .. 4: viterbi_varlen_kernel<NB>, posterior_varlen_kernel<NB>) runs the same batches."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, decode, flipflopfings, synth
from tests import basecall_support as bs

T, NBASES = 130, [1, 2, 3, 4]
LENGTHS = [130, 129, 65, 64, 63, 1, 0]          # both sides of the 64-step traceback batch, the ends, an empty column


def forward_backward(scores, lengths):
    """float64, log domain: (trans, logz) of d logZ / d scores for column n over its first lengths[n] rows (paths start
    in a flip state and end anywhere: decode.py:42-72 / layers.py:1277-1299); rows beyond are 0."""
    Tn, N, S = scores.shape
    nb = int(round((-1 + np.sqrt(1 + 2 * S)) / 2))
    ns = 2 * nb
    to = np.concatenate([np.repeat(np.arange(nb), ns), nb + np.arange(ns) % nb])
    frm = np.concatenate([np.tile(np.arange(ns), nb), np.arange(ns)])
    trans, logz = np.zeros((Tn, N, S)), np.zeros(N)

    def lse(v, axis=0):
        m = v.max(axis, keepdims=True)
        return m.squeeze(axis) + np.log(np.exp(v - m).sum(axis))

    for n, L in enumerate(lengths):
        sc = scores[:L, n].astype(np.float64)
        fwd = np.full((L + 1, ns), -1e30)
        fwd[0, :nb] = 0.0
        for t in range(L):
            v = fwd[t, frm] + sc[t]
            # into flip b: transitions b ns .. b ns + ns - 1; into flop b: nb ns + b (from flip b) and nb ns + nb + b (stay)
            fwd[t + 1, :nb] = lse(v[:nb * ns].reshape(nb, ns), 1)
            fwd[t + 1, nb:] = lse(v[nb * ns:].reshape(2, nb))
        bwd = np.zeros((L + 1, ns))
        for t in range(L, 0, -1):
            # out of state s: transitions b ns + s into every flip b, then nb ns + s into its flop
            bwd[t - 1] = lse((sc[t - 1] + bwd[t, to]).reshape(nb + 1, ns))
        logz[n] = lse(fwd[L])
        trans[:L, n] = np.exp(fwd[:L, frm] + sc + bwd[1:, to] - logz[n])
    return trans, logz


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
NAMES = {"tk_basecall_gather_columns_dev", "tk_decode_varlen_workspace_bytes", "tk_flipflop_viterbi_varlen_dev",
         "tk_flipflop_posterior_varlen_dev"}


def test_library_exports_exactly_what_its_header_declares():
    _lib.build()
    hdr = re.sub(r"/\*.*?\*/", "", open(_lib.DECODE_VARLEN_HEADER).read(), flags=re.S)
    declared = set(re.findall(r"^(?:const\s+)?[a-z_0-9]+\s+\*?\s*([a-z_0-9]+)\(", hdr, flags=re.M))
    assert declared == NAMES
    out = subprocess.run(["nm", "-D", "--defined-only", os.path.join(_lib.CSRC, _lib.DECODE_VARLEN_LIBNAME)],
                         capture_output=True, text=True, check=True).stdout
    assert {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW"} == declared
    assert set(_lib.DECODE_VARLEN_SIGNATURES) == declared
    taken = set(_lib.SIGNATURES) | set(_lib.BASECALL_SIGNATURES) | set(_lib.VARLEN_SIGNATURES) | set(_lib.WGRAD_SIGNATURES)
    assert not declared & taken                                 # the pinned headers declare none of them


def test_binding_has_the_headers_argument_types():
    vp, sz, i = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int
    assert _lib.DECODE_VARLEN_SIGNATURES == {
        "tk_basecall_gather_columns_dev": (i, [vp, vp, sz, sz, vp, vp, vp, sz, sz, vp, vp, vp, vp]),
        "tk_decode_varlen_workspace_bytes": (sz, [sz, sz, sz]),
        "tk_flipflop_viterbi_varlen_dev": (i, [vp, vp, sz, sz, sz, vp, vp, sz, vp]),
        "tk_flipflop_posterior_varlen_dev": (i, [vp, vp, sz, sz, sz, vp, vp, vp, sz, vp, vp]),
    }
    V = _lib.decode_varlen_lib()                                # resolves every symbol
    # 8 traceback bytes (Viterbi) or 8 forward floats (posterior) per row and column; never 0 where the kernels run
    assert V.tk_decode_varlen_workspace_bytes(1000, 64, 4) == 1000 * 64 * 32
    assert V.tk_decode_varlen_workspace_bytes(0, 0, 1) > 0
    assert V.tk_decode_varlen_workspace_bytes(10, 2, 0) == 0 and V.tk_decode_varlen_workspace_bytes(10, 2, 5) == 0


@pytest.mark.parametrize("op", [decode.flipflop_viterbi_path, decode.flipflop_make_trans])
def test_lengths_are_checked_before_anything_is_launched(op):
    x = torch.zeros(T, 2, 40)
    for bad in ([T + 1, 0], [T], [T, 1, 1], [-1, 0], [1.5, 2.0], "ab", torch.tensor([[1, 2]])):
        with pytest.raises(ValueError, match="lengths"):
            op(x, lengths=bad)
    with pytest.raises(RuntimeError, match="no CPU fallback"):   # good lengths: the operator itself has no CPU form
        op(x, lengths=[T, 0])


def test_float64_restatement_agrees_with_the_oracle_at_full_length(oracle_mod):
    sc = synth.crf_case(96, 6, 5)["scores"]
    logz, grad = oracle_mod.flipflop_logz_grad(sc)
    trans, lz = forward_backward(sc, [96] * 6)
    assert np.abs(trans - grad).max() <= 1e-6 and np.abs(lz - logz).max() <= 1e-6 * np.abs(logz).max()
    assert np.abs(trans.sum(2) - 1).max() < 1e-12               # a row of posterior probabilities
    # a shorter column is the column cut, rows beyond are 0, and an empty one has logZ = log(nbase)
    cut, lz = forward_backward(sc, [96, 40, 0, 1, 96, 96])
    assert np.array_equal(cut[:, 0], trans[:, 0]) and not cut[40:, 1].any() and not cut[:, 2].any()
    assert np.abs(cut[:40, 1] - forward_backward(sc[:40, 1:2], [40])[0][:, 0]).max() == 0
    assert lz[2] == pytest.approx(np.log(4))


# ----------------------------------------------------------------------------------------------------------------------
# GPU
# ----------------------------------------------------------------------------------------------------------------------
def _scores(n, seed, nbase=4):
    """Half the columns a trained network's confident scores, half a fresh one's."""
    inp = synth.crf_case(T, n, seed, nbase=nbase, seqlens=np.full(n, 40, dtype=np.int32))
    plain = inp["scores"].copy()
    sharp = synth.confident_scores(inp, seed + 1, nbase=nbase)["scores"]
    sharp[:, 1::2] = plain[:, 1::2]
    return np.ascontiguousarray(sharp)


BATCHES = {"seven": (LENGTHS, 11), "one": ([2], 12)}


def _over_alphabets(*cases):
    """Every case at every alphabet size; the nbase = 4 cases keep the ids they had before the others joined them."""
    return [pytest.param(*c, nb, id="-".join(str(v) for v in c) + ("" if nb == 4 else "-nb%d" % nb))
            for nb in reversed(NBASES) for c in cases]


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _viterbi_abi(sc, lengths):
    """tk_flipflop_viterbi_varlen_dev on NaN-like filled outputs (int64: a pattern no state has)."""
    V, dev = _lib.decode_varlen_lib(), sc.device
    Tn, N, S = sc.shape
    NBASE = flipflopfings.nbase_flipflop(S)
    path = torch.full((Tn + 1, N), -7777, dtype=torch.int64, device=dev)
    wsb = V.tk_decode_varlen_workspace_bytes(Tn, N, NBASE)
    ws = torch.full((wsb,), 0xAB, dtype=torch.uint8, device=dev)
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    assert V.tk_flipflop_viterbi_varlen_dev(_p(sc), _p(lens), Tn, N, NBASE, _p(path), _p(ws), wsb, None) == 0
    return path


def _posterior_abi(sc, lengths):
    V, dev = _lib.decode_varlen_lib(), sc.device
    Tn, N, S = sc.shape
    NBASE = flipflopfings.nbase_flipflop(S)
    trans = torch.full_like(sc, float("nan"))
    logz = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
    wsb = V.tk_decode_varlen_workspace_bytes(Tn, N, NBASE)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev)            # (float NaN patterns)
    lens = torch.tensor(lengths, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    assert V.tk_flipflop_posterior_varlen_dev(_p(sc), _p(lens), Tn, N, NBASE, _p(trans), _p(logz), _p(ws), wsb,
                                              _p(status), None) == 0
    return trans, logz, int(status.item())


@pytest.mark.gpu
@pytest.mark.parametrize("batch,nbase", _over_alphabets(*((b,) for b in BATCHES)))
def test_viterbi_columns_equal_the_column_alone(gpu_device, batch, nbase):
    lengths, seed = BATCHES[batch]
    sc = torch.from_numpy(_scores(len(lengths), seed, nbase)).to(gpu_device)
    path = _viterbi_abi(sc, lengths)
    assert torch.equal(path, decode.flipflop_viterbi_path(sc, lengths=lengths))       # the operator is the entry point
    assert torch.equal(path, decode.flipflop_viterbi_path(sc, lengths=torch.tensor(lengths, device=gpu_device)))
    for n, L in enumerate(lengths):
        assert bool((path[L:, n] == path[L, n]).all()), (n, L)
        if L == 0:                                              # (the fixed-length operator takes no empty tensor)
            assert not path[:, n].any()
            continue
        alone = decode.flipflop_viterbi_path(sc[:L, n:n + 1].contiguous())[:, 0]
        assert torch.equal(path[:L + 1, n], alone), (n, L)
    if len(lengths) > 1:
        # two columns swapped: their results swapped, bit for bit; and again: the same bits
        perm = [2, 1, 0] + list(range(3, len(lengths)))
        swapped = _viterbi_abi(sc[:, perm].contiguous(), [lengths[i] for i in perm])
        assert torch.equal(swapped, path[:, perm]) and torch.equal(_viterbi_abi(sc, lengths), path)
        # full-length columns: the existing operator on the whole batch
        assert torch.equal(_viterbi_abi(sc, [T] * len(lengths)), decode.flipflop_viterbi_path(sc))
        # lengths outside [0, nblk] are clamped
        assert torch.equal(_viterbi_abi(sc, [T + 5, -3] + lengths[2:]), _viterbi_abi(sc, [T, 0] + lengths[2:]))


@pytest.mark.gpu
@pytest.mark.parametrize("batch,sharpen,nbase", _over_alphabets(("seven", 1.0), ("seven", 2.5), ("one", 1.0)))
def test_posterior_columns_against_float64(gpu_device, batch, sharpen, nbase):
    """Per column, in max-norm: |got - ref| <= 2 |alone - ref| + 2e-6 max|ref| (the rule of tests/test_gru_hip.py and
    tests/test_forward_varlen.py): ref the float64 restatement above, alone the existing operator on the column."""
    lengths, seed = BATCHES[batch]
    host = _scores(len(lengths), seed, nbase) * np.float32(sharpen)
    sc = torch.from_numpy(host).to(gpu_device)
    trans, logz, status = _posterior_abi(sc, lengths)
    assert status == 0 and bool(torch.isfinite(trans).all()) and bool(torch.isfinite(logz).all())
    assert torch.equal(trans, decode.flipflop_make_trans(sc, lengths=lengths))
    ref, ref_lz = forward_backward(host, lengths)
    got, ok = trans.cpu().numpy(), True
    for n, L in enumerate(lengths):
        assert not got[L:, n].any(), (n, L)                       # exactly 0
        if L == 0:
            continue
        alone = decode.flipflop_make_trans(sc[:L, n:n + 1].contiguous())[:, 0].cpu().numpy()
        e_got, e_alone = np.abs(got[:L, n] - ref[:L, n]).max(), np.abs(alone - ref[:L, n]).max()
        bound = 2 * e_alone + 2e-6 * np.abs(ref[:L, n]).max()
        print("nbase %d column %d (%d rows, x%.1f): batched %.3g, alone %.3g, bound %.3g" % (nbase, n, L, sharpen, e_got, e_alone, bound))
        ok &= bool(e_got <= bound)
    assert ok
    # logZ: float32 of a sum of up to 130 terms of magnitude <= 12.5
    assert np.abs(logz.cpu().numpy() - ref_lz).max() <= 1e-6 * max(np.abs(ref_lz).max(), 1.0)
    if len(lengths) > 1:
        perm = [2, 1, 0] + list(range(3, len(lengths)))
        swapped = _posterior_abi(sc[:, perm].contiguous(), [lengths[i] for i in perm])
        assert torch.equal(swapped[0], trans[:, perm]) and torch.equal(swapped[1], logz[perm])


@pytest.mark.gpu
def test_posterior_flags_a_non_finite_result(gpu_device):
    for nbase in reversed(NBASES):
        host = _scores(2, 13, nbase)
        host[7, 1, 3] = np.nan
        trans, logz, status = _posterior_abi(torch.from_numpy(host).to(gpu_device), [T, T])
        assert status & _lib.DEFINES["TK_STATUS_NONFINITE_GRAD"] and status & _lib.DEFINES["TK_STATUS_NONFINITE_SCORE"], nbase
        assert bool(torch.isfinite(trans[:, 0]).all()) and bool(torch.isfinite(logz[0])), nbase     # the neighbour is untouched


def _gather_abi(sigs, shift, scale, read_index, tmax, dev):
    V = _lib.decode_varlen_lib()
    lens = np.array([len(s) for s in sigs], dtype=np.int64)
    flat = torch.from_numpy(np.concatenate(sigs).astype(np.float32)).to(dev)
    off = torch.from_numpy(np.concatenate([[0], np.cumsum(lens)])).to(dev)
    sh, scl = (torch.from_numpy(np.asarray(v, dtype=np.float32)).to(dev) for v in (shift, scale))
    idx = torch.tensor(read_index, dtype=torch.int32, device=dev)
    cols = torch.full((tmax, len(read_index), 1), float("nan"), dtype=torch.float32, device=dev)
    out_len = torch.full((len(read_index),), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    assert V.tk_basecall_gather_columns_dev(_p(flat), _p(off), len(sigs), int(lens.sum()), _p(sh), _p(scl), _p(idx),
                                            len(read_index), tmax, _p(cols), _p(out_len), _p(status), None) == 0
    return cols.cpu().numpy(), out_len.cpu().numpy(), int(status.item())


@pytest.mark.gpu
def test_gather_columns_is_bit_equal_to_numpy(gpu_device):
    names = ["len4999", "len2", "len1"]
    sigs = [bs.signal(n) for n in names]
    shift = [np.float32(88.5 + i) for i in range(3)]
    scale = [np.float32(9.75 + 0.5 * i) for i in range(3)]
    index = [2, 0, 1]
    cols, lens, status = _gather_abi(sigs, shift, scale, index, 4999, gpu_device)
    assert status == 0 and lens.tolist() == [1, 4999, 2] and cols.shape == (4999, 3, 1)
    for j, r in enumerate(index):
        want = ((sigs[r] - shift[r]) / scale[r]).astype(np.float32)
        assert cols[:len(want), j, 0].tobytes() == want.tobytes(), names[r]
        assert not cols[len(want):, j].any() and not np.signbit(cols[len(want):, j]).any()
    # a read the normalisation refused (NaN scale, NaN shift): an all-zero column of its length; its neighbours as before
    z, zl, status = _gather_abi(sigs, [shift[0], np.nan, shift[2]], [np.nan, scale[1], scale[2]], index, 4999, gpu_device)
    assert status == 0 and zl.tolist() == [1, 4999, 2] and not z[:, 1].any() and not z[:, 2].any()
    assert z[:, 0].tobytes() == cols[:, 0].tobytes()
    # a read longer than tmax, and an index that names no read: reported, and nothing read or written out of place
    c, cl, status = _gather_abi(sigs, shift, scale, [0, 7, 1], 100, gpu_device)
    assert status == 256 and cl.tolist() == [100, 0, 2] and not c[:, 1].any()
    assert c[:, 0, 0].tobytes() == ((sigs[0] - shift[0]) / scale[0]).astype(np.float32)[:100].tobytes()
