"""The log-partition with a time length per column on the transfer-matrix kernels (include/taiyaki_amd_logz_varlen.h).  A
case is named by what tk_lab_logz_plan reports for its shape (rows per chunk, transfer form, chunks per super): the smallest
(nblk, nbatch) with two or more 64-column groups, one partial, that reach each.  Scores as in tests/test_decode_varlen.py."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, ctc, flipflopfings, layers, synth
from tests.test_decode_instantiations import _lab_logz_plan
from tests.test_loss_varlen import FORMS, NBLK, expected, lengths_for, ragged_case, run

COOP, RING, PLAIN, STREAM = 0, 1, 2, 3
# name -> (nblk, nbatch, (CH, transfer, SUP)); 16-row chunks need ceil(N / 64) * ceil(T / 16) >= 384, the ring 640 chunks, one
# wave per chunk more than 900, its streaming loads more than 300 MB of scores, 16-chunk supers more than 128 chunks
CASES = {"ch8-coop-sup8": (131, 70, (8, COOP, 8)), "ch8-coop-sup16": (1030, 70, (8, COOP, 16)),
         "ch8-ring-sup8": (1024, 300, (8, RING, 8)), "ch8-ring-sup16": (2560, 70, (8, RING, 16)),
         "ch16-coop-sup8": (2048, 130, (16, COOP, 8)), "ch16-coop-sup16": (3060, 70, (16, COOP, 16)),
         "ch16-ring-sup16": (5120, 70, (16, RING, 16)), "ch16-plain-sup16": (7210, 70, (16, PLAIN, 16)),
         "ch16-stream-sup16": (7210, 275, (16, STREAM, 16))}
SMALLEST = "ch8-coop-sup8"
PARAMS = [pytest.param(c, 4, id=c) for c in CASES] + [pytest.param(SMALLEST, nb, id="%s-nb%d" % (SMALLEST, nb)) for nb in (3, 2, 1)]


def forward_backward(scores, lengths):
    """Plain float64, log domain, every column over its own rows: (d logZ / d scores, logZ); rows beyond a length are 0."""
    T, N, S = scores.shape
    nb = flipflopfings.nbase_flipflop(S)
    ns, L, sc = 2 * nb, np.asarray(lengths), scores.astype(np.float64)
    to = np.concatenate([np.repeat(np.arange(nb), ns), nb + np.arange(ns) % nb])
    frm = np.concatenate([np.tile(np.arange(ns), nb), np.arange(ns)])

    def lse(v, axis):
        m = v.max(axis, keepdims=True)
        return m.squeeze(axis) + np.log(np.exp(v - m).sum(axis))
    fwd = np.full((T + 1, N, ns), -1e30)
    fwd[0, :, :nb] = 0.0
    with np.errstate(invalid="ignore"):
        for t in range(T):
            v = fwd[t][:, frm] + sc[t]
            new = np.concatenate([lse(v[:, :nb * ns].reshape(N, nb, ns), 2), lse(v[:, nb * ns:].reshape(N, 2, nb), 1)], 1)
            fwd[t + 1] = np.where((t < L)[:, None], new, fwd[t])
        logz, bwd, trans = lse(fwd[T], 1), np.zeros((N, ns)), np.zeros((T, N, S))
        for t in range(T - 1, -1, -1):
            live = (t < L)[:, None]
            trans[t] = np.where(live, np.exp(fwd[t][:, frm] + sc[t] + bwd[:, to] - logz[:, None]), 0.0)
            bwd = np.where(live, lse((sc[t] + bwd[:, to]).reshape(N, nb + 1, ns), 1), bwd)
    return trans, logz


def test_float64_helper_agrees_with_the_oracle_at_full_length(oracle_mod):
    sc = synth.crf_case(96, 6, 5)["scores"]
    logz, grad = oracle_mod.flipflop_logz_grad(sc)
    trans, lz = forward_backward(sc, [96] * 6)
    assert np.abs(trans - grad).max() <= 1e-6 and np.abs(lz - logz).max() <= 1e-6 * np.abs(logz).max()
    assert forward_backward(sc, [96, 0, 96, 96, 96, 96])[1][1] == pytest.approx(np.log(4))


@functools.lru_cache(maxsize=2)
def scores_of(case, nbase):
    T, N, _ = CASES[case]
    n = min(N, 130)                     # (wider batches repeat these columns)
    inp = synth.crf_case(T, n, 11, nbase=nbase, seqlens=np.full(n, 40, dtype=np.int32))
    sharp = synth.confident_scores(inp, 12, nbase=nbase)["scores"]
    sharp[:, 1::2] = inp["scores"][:, 1::2]
    return np.ascontiguousarray(np.tile(sharp, (1, -(-N // n), 1))[:, :N])


def ragged_lengths(case, seed):
    """0, 1, CH - 1, CH, CH + 1, a multiple of CH SUP, nblk - 1, nblk over the groups, and one whole group (the first, the
    partial last one for every other case) in which every column is shorter than nblk / 2."""
    T, N, (ch, _, sup) = CASES[case]
    rs = np.random.RandomState(seed)
    lens = rs.randint(0, T + 1, size=N)
    ngrp = -(-N // 64)
    short = (ngrp - 1) if list(CASES).index(case) % 2 else 0
    other = 64 * (1 if short == 0 else 0)
    lens[64 * short:64 * short + 64] = rs.randint(0, (T - 1) // 2, size=len(lens[64 * short:64 * short + 64]))
    lens[64 * short:64 * short + 2] = [0, 1]
    lens[other:other + 6] = [ch - 1, ch, ch + 1, (T // (ch * sup)) * ch * sup, T - 1, T]
    assert lens[64 * short:64 * short + 64].max() < T / 2 and len(lens) == N
    return lens


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def logz_abi(sc, lengths, varlen=True, want_trans=True):
    """tk_flipflop_logz_varlen_dev (varlen False: tk_flipflop_logz_dev) on outputs and a workspace filled with NaN patterns
    -> trans, logz, the status word.  lengths None: the NULL pointer."""
    V, dev = (_lib.logz_varlen_lib() if varlen else _lib.lib()), sc.device
    T, N, S = sc.shape
    nbase = flipflopfings.nbase_flipflop(S)
    trans = torch.full_like(sc, float("nan")) if want_trans else None
    logz = torch.full((N,), float("nan"), dtype=torch.float32, device=dev)
    wsb = V.tk_flipflop_logz_varlen_workspace_bytes(T, N, nbase) if varlen else V.tk_flipflop_logz_workspace_bytes(T, N, nbase)
    ws = torch.full((wsb,), 0xFF, dtype=torch.uint8, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    if varlen:
        lens = None if lengths is None else torch.as_tensor(np.asarray(lengths), dtype=torch.int32).to(dev)
        rc = V.tk_flipflop_logz_varlen_dev(_p(sc), _p(lens), T, N, nbase, _p(trans), _p(logz), _p(ws), wsb, _p(status), None)
    else:
        rc = V.tk_flipflop_logz_dev(_p(sc), T, N, nbase, _p(logz), _p(trans), _p(ws), wsb, _p(status), None)
    assert rc == 0, rc
    return trans, logz, int(status.item())


@pytest.mark.gpu
@pytest.mark.parametrize("case,nbase", PARAMS)
def test_full_lengths_are_the_fixed_length_operator_bit_for_bit(gpu_device, case, nbase):
    T, N, form = CASES[case]
    assert _lab_logz_plan(T, N, nbase)[:3] == form
    sc = torch.from_numpy(scores_of(case, nbase)).to(gpu_device)
    want = logz_abi(sc, None, varlen=False)
    assert want[2] == 0
    for lengths in (None, [T] * N):
        got = logz_abi(sc, lengths)
        assert got[2] == 0 and torch.equal(got[1], want[1]) and torch.equal(got[0], want[0]), (case, lengths is None)
    # the log-partition alone: no posterior launch, the same values
    assert torch.equal(logz_abi(sc, [T] * N, want_trans=False)[1], want[1])


@pytest.mark.gpu
@pytest.mark.parametrize("case,nbase", [p for p in PARAMS if p.values[0] != "ch16-stream-sup16"])
def test_ragged_lengths_against_float64(gpu_device, case, nbase):
    """Per column in max-norm: |got - ref| <= 2 |alone - ref| + 2e-6 max|ref| (the rule of tests/test_decode_varlen.py and
    tests/test_gru_hip.py), logZ likewise with the floor 1e-6 max(|ref|, 1): ref the float64 helper above, alone the
    fixed-length operator on scores[:T_n, n:n+1]."""
    T, N, form = CASES[case]
    assert _lab_logz_plan(T, N, nbase)[:3] == form
    lens = ragged_lengths(case, 5)
    host = scores_of(case, nbase).copy()
    ref, ref_lz = forward_backward(host, lens)
    host[np.arange(T)[:, None] >= lens[None, :]] = np.nan          # nothing beyond a length may reach an output
    sc = torch.from_numpy(host).to(gpu_device)
    trans, logz, status = logz_abi(sc, lens)
    assert status == 0 and bool(torch.isfinite(trans).all()) and bool(torch.isfinite(logz).all())
    got, got_lz = trans.cpu().numpy(), logz.cpu().numpy()
    for n, L in enumerate(lens):
        assert not got[L:, n].any(), (n, L)                         # exactly 0
        if L == 0:
            assert abs(got_lz[n] - np.log(nbase)) <= 1e-6
            continue
        alone_lz, alone = layers._logz_launch(sc[:L, n:n + 1].contiguous(), True)
        alone, alone_lz = alone[:, 0].cpu().numpy(), float(alone_lz[0])
        e, e_alone = np.abs(got[:L, n] - ref[:L, n]).max(), np.abs(alone - ref[:L, n]).max()
        z, z_alone = abs(got_lz[n] - ref_lz[n]), abs(alone_lz - ref_lz[n])
        bound, zbound = 2 * e_alone + 2e-6 * np.abs(ref[:L, n]).max(), 2 * z_alone + 1e-6 * max(abs(ref_lz[n]), 1.0)
        assert e <= bound and z <= zbound, (case, n, L, e, e_alone, bound, z, z_alone, zbound)
    # a second run repeats every bit; lengths outside [0, nblk] are clamped
    again = logz_abi(sc, lens)
    assert torch.equal(again[0], trans) and torch.equal(again[1], logz)
    wild = np.where(lens == T, T + 5, np.where(lens == 0, -3, lens))
    clamped = logz_abi(sc, wild)
    assert (wild != lens).sum() >= 2 and torch.equal(clamped[0], trans) and torch.equal(clamped[1], logz)
    # a column of the first group swapped with one of the second, lengths included: the two results swap, bit for bit
    perm = np.arange(N)
    perm[[3, 67]] = [67, 3]
    swapped = logz_abi(sc[:, perm].contiguous(), lens[perm])
    assert torch.equal(swapped[0], trans[:, perm]) and torch.equal(swapped[1], logz[perm])


@pytest.mark.gpu
def test_logpartition_operator_is_the_entry_point(gpu_device, monkeypatch):
    monkeypatch.setattr(layers, "USE_HIP_LOGZ_VARLEN", True)
    T, N, _ = CASES[SMALLEST]
    lens = ragged_lengths(SMALLEST, 6)
    sc = torch.from_numpy(scores_of(SMALLEST, 4)).to(gpu_device)
    trans, logz, _ = logz_abi(sc, lens)
    before = dict(layers.logz_varlen_calls)
    x = sc.clone().requires_grad_()
    out = layers.flipflop_logpartition(x, lengths=lens)
    out.sum().backward()
    assert layers.logz_varlen_calls["logz"] == before["logz"] + 1
    assert torch.equal(out.detach(), logz) and torch.equal(x.grad, trans)
    assert torch.equal(layers.flipflop_logpartition(sc, lengths=torch.from_numpy(lens).to(gpu_device)), logz)  # logZ alone


@pytest.mark.gpu
@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("form", ["plain", "catmod"])
def test_fused_loss_against_the_oracle(oracle_mod, gpu_device, monkeypatch, form, second):
    """ctc.flipflop_mean_loss(..., lengths=) with the switch on, at the lengths and under the bounds of
    tests/test_loss_varlen.py's fused cases: loss rtol 1e-5 / atol 2e-6, gradient 2e-5 x the read's weight; expected values
    from the oracle one column at a time."""
    monkeypatch.setattr(layers, "USE_HIP_LOGZ_VARLEN", True)
    inp = ragged_case(NBLK, lengths_for(FORMS[form, 1.0], second), 50, form == "catmod")
    N = len(inp["lengths"])
    wloss, wg32, _ = expected(oracle_mod, inp, 1.0, fused=True)
    before = layers.logz_varlen_calls["loss"]
    lv, fg, retried, redone = run(inp, 1.0, gpu_device, fused=True)
    assert layers.logz_varlen_calls["loss"] == before + 1 and (retried, redone) == (0, 0)
    np.testing.assert_allclose(lv, wloss, rtol=1e-5, atol=2e-6)
    err = np.abs(fg - wg32 / N).max(axis=(0, 2)) * N
    assert np.isfinite(fg).all() and (err <= 2e-5).all(), err
    assert not fg[np.arange(NBLK)[:, None] >= inp["lengths"][None, :]].any() and not lv[inp["lengths"] == 0].any()
    assert ctc.last_retry_count() == 0 and ctc.last_gate_count() == 0
