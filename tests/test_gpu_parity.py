"""GPU parity tests proper: HIP kernels (through the Python operator API -> C ABI)
against the pinned CPU oracle and the reference-generated golden fixtures.

Tolerances (BASELINE.json north_star): loss / logZ <= 1e-4 relative (asserted at
1e-5, observed ~1e-6); logZ gradients (posteriors) <= 2e-5 absolute; CRF / cat-mod gradients
(posteriors / T) <= 5e-4 / T absolute, i.e. 5e-4 of full scale whatever T is;
Viterbi fwd / traceback / path bit-exact.
"""
import ctypes

import numpy as np
import pytest
import torch

from tests import parity
from tests.conftest import load_golden
from tests.golden import cases

pytestmark = pytest.mark.gpu

LOSS_RTOL = 1e-5
GRAD_ATOL = 2e-5        # logZ gradients (posteriors in [0, 1]); an outer bound for CRF gradients
# CRF / cat-mod gradients are posteriors / T (x the weight in a modification column): the element-wise
# bound that means something is on that scale -- 5e-4 of a posterior's full scale at EVERY T, against the
# float64 witness of the recursion; against the fp32 oracle the reference's own rounding noise is added
# (parity.crf_grad_ok, parity.compare_crf)
GRAD_T_ATOL = parity.GRAD_T_ATOL


def _check_grad_golden(gold, prefix, grad, atol):
    if prefix in gold.files:
        np.testing.assert_allclose(grad, gold[prefix], atol=atol, rtol=0)
    else:
        cs = cases.grad_checksums(grad)
        np.testing.assert_allclose(cs["sum"], gold[prefix + "_sum"], rtol=1e-4, atol=1e-4)
        np.testing.assert_allclose(cs["sumsq"], gold[prefix + "_sumsq"], rtol=1e-3, atol=1e-7)
        np.testing.assert_allclose(cs["sample"], gold[prefix + "_sample"], atol=atol, rtol=0)


# ---------------------------------------------------------------- (A) CRF ----
@pytest.mark.parametrize("name", list(cases.CRF_SMALL))
def test_crf_small(oracle_mod, gpu_device, name):
    spec = cases.CRF_SMALL[name]
    inp = cases.crf_inputs(spec)
    r = parity.compare_crf(oracle_mod, inp, spec["sharp"], gpu_device)
    assert r["finite"]
    assert r["loss_rel"] < LOSS_RTOL, r["loss_rel"]
    assert r["grad_abs"] < GRAD_ATOL, r["grad_abs"]
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])
    assert r["rowsum_dev"] < 1e-4
    gold = load_golden("crf_small.npz")
    np.testing.assert_allclose(r["loss"], gold[name + "/loss"], rtol=LOSS_RTOL, atol=1e-6)
    _check_grad_golden(gold, name + "/grad", r["grad"], GRAD_T_ATOL / spec["T"])
    # forward-only path (no requires_grad): reference returns the forward score
    loss_ng, _ = parity.run_crf(inp, spec["sharp"], gpu_device, want_grad=False)
    np.testing.assert_allclose(loss_ng, gold[name + "/loss_nograd"], rtol=LOSS_RTOL, atol=1e-6)


@pytest.mark.parametrize("name", list(cases.CATMOD_SMALL))
def test_catmod_small(oracle_mod, gpu_device, name):
    spec = cases.CATMOD_SMALL[name]
    inp = cases.crf_inputs(spec, cases.NMODS)
    r = parity.compare_crf(oracle_mod, inp, spec["sharp"], gpu_device)
    assert r["finite"]
    assert r["loss_rel"] < LOSS_RTOL, r["loss_rel"]
    assert r["grad_abs"] < 4 * GRAD_ATOL, r["grad_abs"]     # mod bins carry p * 8.0
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])
    gold = load_golden("catmod_small.npz")
    np.testing.assert_allclose(r["loss"], gold[name + "/loss"], rtol=LOSS_RTOL, atol=1e-6)
    _check_grad_golden(gold, name + "/grad", r["grad"], GRAD_T_ATOL / spec["T"])


def test_crf_seqs_on_device(oracle_mod, gpu_device):
    """train_abinitio.py:207-210 passes seqs / seqlens as GPU tensors."""
    spec = cases.CRF_SMALL["t64n8"]
    inp = cases.crf_inputs(spec)
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device, seq_on_device=True)
    assert r["loss_rel"] < LOSS_RTOL and r["grad_abs"] < GRAD_ATOL


def test_ctc_loss_reference_unit_test(oracle_mod, gpu_device):
    """test/unit/test_ctc_loss.py:80-135 replayed on the HIP operators."""
    from taiyaki_amd import ctc, layers
    ka = load_golden("known_answers.npz")
    outputs = torch.tensor(ka["ctcloss/outputs"], device=gpu_device)
    assert abs(float(layers.flipflop_logpartition(outputs)[0])) < 1e-5
    for name in ("015", "237"):
        x = outputs.clone().requires_grad_()
        lv = ctc.crf_flipflop_loss(x, torch.tensor(ka["ctcloss/%s_seq" % name]),
                                   torch.tensor([3]), 1.0)
        prob = float(torch.exp(-lv.detach() * outputs.shape[0]))
        assert abs(prob - 0.5) < 1e-6
        lv.sum().backward()
        np.testing.assert_allclose(x.grad.cpu().numpy(), ka["ctcloss/%s_grad" % name], atol=1e-5)
        # finite-difference check of the analytic gradient (test_grad, 105-135)
        torch.manual_seed(0)
        dx = torch.randn_like(outputs) * 1e-3
        lv2 = ctc.crf_flipflop_loss(outputs + dx, torch.tensor(ka["ctcloss/%s_seq" % name]),
                                    torch.tensor([3]), 1.0)
        change = float((lv2 - lv).sum())
        est = float((dx * x.grad).sum())
        assert abs(change - est) / abs(float(lv)) < 1e-4


def test_c_harness_known_answers_host_abi(oracle_mod, gpu_device):
    """The reference's embedded harness data through the EXACT reference prototypes
    (host pointers) of the shared library: -2.378088 ; -52.354622, -195.435257."""
    from taiyaki_amd import _lib
    L = _lib.lib()
    ka = load_golden("known_answers.npz")
    f32p, szp, i32p = (ctypes.POINTER(ctypes.c_float), ctypes.POINTER(ctypes.c_size_t),
                       ctypes.POINTER(ctypes.c_int32))

    def p(a, t):
        return ctypes.cast(a.ctypes.data, ctypes.c_void_p)

    lp = np.ascontiguousarray(ka["ccrf/logprob"], dtype=np.float32)
    move = np.ascontiguousarray(ka["ccrf/move"], dtype=np.uintp)
    stay = np.ascontiguousarray(ka["ccrf/stay"], dtype=np.uintp)
    seqlen = np.ascontiguousarray(ka["ccrf/seqlen"], dtype=np.int32)
    score = np.zeros(2, dtype=np.float32)
    grad = np.zeros_like(lp)
    L.crf_flipflop_grad(p(lp, f32p), 40, 7, 2, p(move, szp), p(stay, szp), p(seqlen, i32p),
                        p(score, f32p), p(grad, f32p))
    np.testing.assert_allclose(score, ka["ccrf/score"], atol=5e-6)
    np.testing.assert_allclose(grad[:, 0], grad[:, 1], atol=1e-6)
    np.testing.assert_allclose(grad.sum(axis=2), 1.0, atol=1e-5)      # softmax rows
    score2 = np.zeros(2, dtype=np.float32)
    L.crf_flipflop_cost(p(lp, f32p), 40, 7, 2, p(move, szp), p(stay, szp), p(seqlen, i32p),
                        p(score2, f32p))
    np.testing.assert_allclose(score2, ka["ccrf/score"], atol=5e-6)
    if oracle_mod.ref_available():
        rscore = np.zeros(2, dtype=np.float32)
        rgrad = np.zeros_like(lp)
        fn = oracle_mod.ref().crf_flipflop_grad
        fn.restype = None
        fn(p(lp, f32p), ctypes.c_size_t(40), ctypes.c_size_t(7), ctypes.c_size_t(2),
           p(move, szp), p(stay, szp), p(seqlen, i32p), p(rscore, f32p), p(rgrad, f32p))
        np.testing.assert_allclose(grad, rgrad, atol=1e-5)
    # cat-mod harness
    lp = np.ascontiguousarray(ka["ccm/logprob"], dtype=np.float32)
    mm = np.ascontiguousarray(ka["ccm/modmoveidx"], dtype=np.uintp)
    mf = np.ascontiguousarray(ka["ccm/modmovefact"], dtype=np.float32)
    move = np.ascontiguousarray(ka["ccm/move"], dtype=np.uintp)
    stay = np.ascontiguousarray(ka["ccm/stay"], dtype=np.uintp)
    score = np.zeros(2, dtype=np.float32)
    L.cat_mod_flipflop_cost(p(lp, f32p), 45, 7, 2, p(move, szp), p(stay, szp), p(mm, szp),
                            p(mf, f32p), p(seqlen, i32p), p(score, f32p))
    np.testing.assert_allclose(score, ka["ccm/score"], rtol=2e-6)
    grad = np.zeros_like(lp)
    L.cat_mod_flipflop_grad(p(lp, f32p), 45, 7, 2, p(move, szp), p(stay, szp), p(mm, szp),
                            p(mf, f32p), p(seqlen, i32p), p(score, f32p), p(grad, f32p))
    np.testing.assert_allclose(score, ka["ccm/score"], rtol=2e-6)
    if oracle_mod.ref_available():
        # ... and the cat-mod GRADIENT through the exact prototype against the genuine reference C
        rscore = np.zeros(2, dtype=np.float32)
        rgrad = np.zeros_like(lp)
        fn = oracle_mod.ref().cat_mod_flipflop_grad
        fn.restype = None
        fn(p(lp, f32p), ctypes.c_size_t(45), ctypes.c_size_t(7), ctypes.c_size_t(2), p(move, szp), p(stay, szp),
           p(mm, szp), p(mf, f32p), p(seqlen, i32p), p(rscore, f32p), p(rgrad, f32p))
        np.testing.assert_allclose(score, rscore, rtol=2e-6)
        np.testing.assert_allclose(grad, rgrad, atol=1e-5)
        assert float(np.abs(rgrad[:, :, 40:]).max()) > 0        # the mod columns do receive gradient


def test_numpy_level_ctc_functions_on_known_answers(oracle_mod, gpu_device):
    """`taiyaki.ctc.crf_flipflop_cost / _grad`, `cat_mod_flipflop_cost / _grad` (ctc.pyx:31-113,
    162-255) and `taiyaki.layers.log_partition_flipflop` (layers.py:1277-1299) under the REFERENCE's
    names after `shim.install()`: the C harness data give -score / nblk of the reference's known
    answers, the move / stay ids of `flipflopfings` reproduce the operator, and the way the
    reference's own `FlipFlopCRF.forward` calls them (ctc.pyx:119-145) gives the operator's loss."""
    from taiyaki_amd import shim
    ka = load_golden("known_answers.npz")
    assert shim.install(force_standalone=True) == "standalone"
    try:
        from taiyaki import ctc as tctc, flipflopfings as tff, layers as tlayers
        lp = np.ascontiguousarray(ka["ccrf/logprob"], dtype=np.float32)
        move = np.ascontiguousarray(ka["ccrf/move"], dtype=np.uintp)
        stay = np.ascontiguousarray(ka["ccrf/stay"], dtype=np.uintp)
        seqlen = np.ascontiguousarray(ka["ccrf/seqlen"], dtype=np.int32)
        nblk = lp.shape[0]
        cost = tctc.crf_flipflop_cost(lp, move, stay, seqlen)
        assert torch.is_tensor(cost) and cost.device.type == "cpu" and cost.shape == (2,)
        np.testing.assert_allclose(-cost.numpy() * nblk, ka["ccrf/score"], atol=5e-6)     # -2.378088
        cost2, grads = tctc.crf_flipflop_grad(lp, move, stay, seqlen, pin=True)
        assert grads.shape == lp.shape      # (`pin` pins the C call's output buffers; -x / nblk is a new tensor, as in ctc.pyx:113)
        np.testing.assert_allclose(cost2.numpy(), cost.numpy(), atol=1e-7)
        np.testing.assert_allclose(-grads.numpy().sum(axis=2) * nblk, 1.0, atol=1e-5)
        lpm = np.ascontiguousarray(ka["ccm/logprob"], dtype=np.float32)
        mm = np.ascontiguousarray(ka["ccm/modmoveidx"], dtype=np.uintp)
        mf = np.ascontiguousarray(ka["ccm/modmovefact"], dtype=np.float32)
        mmove = np.ascontiguousarray(ka["ccm/move"], dtype=np.uintp)
        mstay = np.ascontiguousarray(ka["ccm/stay"], dtype=np.uintp)
        mcost = tctc.cat_mod_flipflop_cost(lpm, mmove, mstay, mm, mf, seqlen)
        np.testing.assert_allclose(-mcost.numpy() * nblk, ka["ccm/score"], rtol=2e-6)     # -52.35, -195.4
        mcost2, mgrads = tctc.cat_mod_flipflop_grad(lpm, mmove, mstay, mm, mf, seqlen)
        np.testing.assert_allclose(mcost2.numpy(), mcost.numpy(), rtol=1e-6)
        assert mgrads.shape == lpm.shape and float(mgrads[:, :, 40:].abs().max()) > 0
        # the reference's own forward (ctc.pyx:119-145) written against these names == the operator
        spec = cases.CRF_SMALL["t64n8"]
        inp = cases.crf_inputs(spec)
        sharp = 1.0
        lp2 = np.ascontiguousarray(inp["scores"] * sharp, dtype=np.float32)
        sl = inp["seqlens"].astype(np.int32)
        off = np.concatenate([[0], np.cumsum(sl)])
        seqs = [inp["seqs"][off[i]:off[i + 1]] for i in range(len(sl))]
        mv = np.concatenate([tff.move_indices(s) for s in seqs if len(s)]).astype(np.uintp)
        st = np.concatenate([tff.stay_indices(s) for s in seqs]).astype(np.uintp)
        c3, g3 = tctc.crf_flipflop_grad(lp2, mv, st, sl)
        x = torch.tensor(inp["scores"], device=gpu_device, requires_grad=True)
        lv = tctc.crf_flipflop_loss(x, torch.tensor(inp["seqs"]), torch.tensor(inp["seqlens"]), sharp)
        lv.sum().backward()
        np.testing.assert_allclose(c3.numpy() / sharp, lv.detach().cpu().numpy(), rtol=LOSS_RTOL, atol=2e-6)
        T = lp2.shape[0]
        assert float(np.abs(g3.numpy() - x.grad.cpu().numpy()).max()) * T < 5e-4
        oloss, ograd = oracle_mod.crf_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], sharp)
        np.testing.assert_allclose(c3.numpy(), oloss, rtol=LOSS_RTOL, atol=2e-6)
        assert float(np.abs(g3.numpy() - ograd).max()) * T < 5e-4
        # logZ with the reference's (N, 1) shape: test_ctc_loss.py:85, test_decodeutil.py:20
        outputs = torch.tensor(ka["ctcloss/outputs"], device=gpu_device)
        lz = tlayers.log_partition_flipflop(outputs)
        assert lz.shape == (outputs.shape[1], 1) and abs(float(lz)) < 1e-5
        assert torch.equal(lz.squeeze(1), tlayers.flipflop_logpartition(outputs))
        # a path the labels cannot take gives -inf scores in the reference: same AssertionError
        bad = np.full_like(lp, -3e38)
        with pytest.raises(AssertionError, match="costs must be finite|Gradients not finite"):
            tctc.crf_flipflop_grad(bad, move, stay, seqlen)
    finally:
        shim.uninstall()


# ---------------------------------------------------------- (B) logZ --------
@pytest.mark.parametrize("name", list(cases.LOGZ_SMALL))
def test_logz_small(oracle_mod, gpu_device, name):
    sc = cases.logz_inputs(cases.LOGZ_SMALL[name])
    r = parity.compare_logz(oracle_mod, sc, gpu_device)
    assert r["finite"]
    assert r["logz_rel"] < LOSS_RTOL, r["logz_rel"]
    assert r["nograd_same"] == 0.0
    assert r["grad_abs"] < GRAD_ATOL, r["grad_abs"]
    assert r["rowsum_dev"] < 1e-5
    gold = load_golden("logz_small.npz")
    np.testing.assert_allclose(r["logz"], gold[name + "/logz"], rtol=LOSS_RTOL)
    _check_grad_golden(gold, name + "/grad", r["grad"], GRAD_ATOL)


def test_logz_known_answers(oracle_mod, gpu_device):
    from taiyaki_amd import decode, layers
    ka = load_golden("known_answers.npz")
    w = torch.tensor(ka["decodeutil/weights"][:, None, :], device=gpu_device)
    assert abs(float(layers.flipflop_logpartition(w)[0]) - float(ka["decodeutil/tensor_score"])) < 1e-4
    trans = decode.flipflop_make_trans(torch.tensor(ka["decode/scores"], device=gpu_device))
    np.testing.assert_allclose(trans.cpu().numpy(), ka["decode/trans"], atol=1e-5)


def test_logz_strided_input_and_grad_scaling(oracle_mod, gpu_device):
    """calculate_loss passes outputs[:, :, :ntrans] of a 46-column tensor
    (bin/train_flipflop.py:175-176) and scales by 1/nblk."""
    from taiyaki_amd import layers
    inp = cases.crf_inputs(cases.CATMOD_SMALL["t50n4"], cases.NMODS)
    x = torch.tensor(inp["scores"], device=gpu_device, requires_grad=True)
    lz = layers.flipflop_logpartition(x[:, :, :40]) / 50.0
    (lz * torch.arange(1, 5, device=gpu_device)).sum().backward()
    olz, ograd = oracle_mod.flipflop_logz_grad(np.ascontiguousarray(inp["scores"][:, :, :40]))
    np.testing.assert_allclose(lz.detach().cpu().numpy(), olz / 50.0, rtol=LOSS_RTOL)
    g = x.grad.cpu().numpy()
    assert np.all(g[:, :, 40:] == 0)
    np.testing.assert_allclose(g[:, :, :40], ograd * (np.arange(1, 5) / 50.0)[None, :, None],
                               atol=GRAD_ATOL)


# ---------------------------------------------------------- Viterbi ---------
@pytest.mark.parametrize("name", list(cases.LOGZ_SMALL))
def test_viterbi_small_bit_exact(oracle_mod, gpu_device, name):
    sc = cases.logz_inputs(cases.LOGZ_SMALL[name])
    r = parity.compare_viterbi(oracle_mod, sc, gpu_device)
    assert r["path_mismatch"] == 0 and r["tb_mismatch"] == 0 and r["fwd_bit_mismatch"] == 0
    gold = load_golden("logz_small.npz")
    np.testing.assert_array_equal(r["path"], gold[name + "/path"])
    np.testing.assert_array_equal(r["fwd"][-1], gold[name + "/fwd_last"])


def test_viterbi_reference_unit_test_and_ties(oracle_mod, gpu_device):
    """test/unit/test_decode.py:20-54 expected path; all-zero scores pin the tie rule."""
    ka = load_golden("known_answers.npz")
    fwd, tb, path = parity.run_viterbi(ka["decode/scores"], gpu_device)
    np.testing.assert_array_equal(path[:, 0], ka["decode/expected_path"])
    np.testing.assert_array_equal(tb, ka["decode/tb"])
    np.testing.assert_array_equal(fwd, ka["decode/fwd"])
    fwd, tb, path = parity.run_viterbi(np.zeros((5, 2, 40), dtype=np.float32), gpu_device)
    np.testing.assert_array_equal(tb, ka["ties/tb"])
    np.testing.assert_array_equal(path, ka["ties/path"])
    np.testing.assert_array_equal(fwd, ka["ties/fwd"])


@pytest.mark.parametrize("T", [1, 2, 11, 12, 13, 63, 64, 65, 255, 256, 257, 300, 1037])
def test_viterbi_batch_edges_and_tie_heavy_scores(oracle_mod, gpu_device, T):
    """The kernel runs groups of 12 steps straight-line and decodes the path 64 steps per scan, four
    scans in flight: lengths around those boundaries, on scores quantised to a grid of 0.5 (exact
    ties in nearly every step -> the first-index rule decides, decode.py:99-105) and on continuous
    ones; forward scores, traceback and paths bit for bit, full outputs and path-only."""
    import torch
    from taiyaki_amd import decode
    rng = np.random.RandomState(T)
    for quantised in (True, False):
        sc = rng.randn(T, 11, 40).astype(np.float32) * 2
        if quantised:
            sc = (np.round(sc * 2) / 2).astype(np.float32)
        r = parity.compare_viterbi(oracle_mod, sc, gpu_device)
        assert r["path_mismatch"] == 0 and r["tb_mismatch"] == 0 and r["fwd_bit_mismatch"] == 0, (T, quantised)
        path_only = decode.flipflop_viterbi_path(torch.from_numpy(sc).to(gpu_device)).cpu().numpy()
        np.testing.assert_array_equal(path_only, r["path"])


# ------------------------------------------------ BASELINE.json full sizes ---
@pytest.mark.parametrize("name", list(cases.FULLSIZE))
def test_fullsize_against_reference_goldens(gpu_device, name):
    """cfg 2 / 4 / 5 / row K: per-read loss, logZ, lossvector (calculate_loss
    assembly, bin/train_flipflop.py:172-182), gradient checksums, Viterbi path hash."""
    gold = load_golden("fullsize.npz")
    spec = cases.FULLSIZE[name]
    inp = parity.fullsize_inputs(name)
    loss, grad = parity.run_crf(inp, 1.0, gpu_device)
    # WHICH kernel answered (round-4 verdict): the log-domain redo is also correct, so a regression that
    # disowned every read would stay green here and cost 7x in the loss.  Every configuration on inputs a
    # network can produce keeps all its reads on the linear path; cfg4's raw modification logits x 8 do not.
    from taiyaki_amd import ctc
    raw_logits = spec["mods"] is not None and not spec.get("lsm")
    assert raw_logits or ctc.last_gate_count() == 0, ctc.last_gate_count()
    np.testing.assert_allclose(loss, gold[name + "/loss"], rtol=1e-4)
    assert parity.rel_err(loss, gold[name + "/loss"]) < 2e-5
    cs = cases.grad_checksums(grad)
    np.testing.assert_allclose(cs["sum"], gold[name + "/grad_sum"], rtol=1e-4, atol=1e-4)
    np.testing.assert_allclose(cs["sumsq"], gold[name + "/grad_sumsq"], rtol=2e-3)
    # (on the posterior scale: a modification column's gradient carries its weight, 8 at cfg 4.  Plain CRF:
    # 2e-4 of a posterior's full scale; cfg 4's inputs are RAW U(-5, 5) modification logits times that 8 --
    # log values in the thousands, where the fp32 reference's own posteriors are ~1e-3 from float64 (fuzz
    # lines in profiles/r4_pytest_gpu_*.log) and most reads are redone by the log-domain kernel)
    col = cs["sample_idx"] % grad.shape[2]
    np.testing.assert_array_less(np.abs(cs["sample"] - gold[name + "/grad_sample"]) * parity.posterior_scale(inp)[col],
                                 (1e-3 if raw_logits else 2e-4) / spec["T"])
    # every gradient row of a live read sums to -1/T (posterior is a distribution)
    np.testing.assert_allclose(grad[:, :, :40].sum(axis=2) * spec["T"], -1.0, atol=2e-4)
    del grad
    sc40 = np.ascontiguousarray(inp["scores"][:, :, :40])
    lz, lgrad = parity.run_logz(sc40, gpu_device)
    np.testing.assert_allclose(lz, gold[name + "/logz"], rtol=1e-5)
    cs = cases.grad_checksums(lgrad)
    np.testing.assert_allclose(cs["sum"], gold[name + "/lgrad_sum"], rtol=1e-4)
    np.testing.assert_allclose(cs["sumsq"], gold[name + "/lgrad_sumsq"], rtol=1e-3)
    np.testing.assert_allclose(cs["sample"], gold[name + "/lgrad_sample"], atol=GRAD_ATOL)
    np.testing.assert_allclose(lgrad.sum(axis=2), 1.0, atol=1e-5)
    del lgrad
    np.testing.assert_allclose(loss + lz / spec["T"], gold[name + "/lossvector"], rtol=1e-4)
    _, _, path = parity.run_viterbi(sc40, gpu_device)
    np.testing.assert_array_equal(parity.path_hash(path), gold[name + "/path_hash"])


# ------------------------------------------------ operator-level behaviour ---
def test_loss_assembly_backward_matches_oracle(oracle_mod, gpu_device):
    """loss = mean(crf + logZ/T); backward through both HIP operators at once."""
    from taiyaki_amd import ctc, layers
    inp = cases.crf_inputs(cases.CRF_SMALL["t200n8"])
    T = 200
    x = torch.tensor(inp["scores"], device=gpu_device, requires_grad=True)
    lv = ctc.crf_flipflop_loss(x, torch.tensor(inp["seqs"]), torch.tensor(inp["seqlens"]), 1.0)
    lv = lv + layers.flipflop_logpartition(x) / T
    lv.mean().backward()
    oloss, ograd = oracle_mod.crf_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], 1.0)
    olz, olgrad = oracle_mod.flipflop_logz_grad(inp["scores"])
    np.testing.assert_allclose(lv.detach().cpu().numpy(), oloss + olz / T, rtol=1e-5)
    np.testing.assert_allclose(x.grad.cpu().numpy(), (ograd + olgrad / T) / 8, atol=1e-6)


def test_nonfinite_input_raises_like_reference(gpu_device):
    """ctc.pyx:48,62-65: non-finite => AssertionError."""
    from taiyaki_amd import ctc
    inp = cases.crf_inputs(cases.CRF_SMALL["t50n4"])
    sc = inp["scores"].copy()
    sc[10, 1, :] = np.nan
    x = torch.tensor(sc, device=gpu_device, requires_grad=True)
    with pytest.raises(AssertionError):
        ctc.crf_flipflop_loss(x, torch.tensor(inp["seqs"]), torch.tensor(inp["seqlens"]), 1.0)


def test_cpu_tensor_fails_loudly():
    from taiyaki_amd import ctc, layers
    with pytest.raises(RuntimeError):
        layers.flipflop_logpartition(torch.zeros(4, 1, 40))
    with pytest.raises(RuntimeError):
        ctc.crf_flipflop_loss(torch.zeros(4, 1, 40), torch.tensor([0, 1]), torch.tensor([2]), 1.0)


# ------------------------------------------------ edge cases and invariants ---
def test_ragged_and_degenerate_batches(oracle_mod, gpu_device):
    """Ragged lengths in one batch: L = 1, L = T + 1 (every block must move), a
    zero-length read last (c_crf_flipflop.c:269-272, 458-464), homopolymer runs."""
    from taiyaki_amd import synth
    T, N = 40, 6
    seqlens = np.array([1, T + 1, 17, 40, 2, 0], dtype=np.int32)
    total = int(seqlens.sum())
    bases = np.zeros(total, dtype=np.int64)                 # all-A homopolymers ...
    bases[1:1 + T + 1] = synth.randint(7, 2, T + 1, 4)      # ... except the L = T + 1 read
    seqs = np.concatenate([synth.flipflop_code(bases[o:o + L]) for o, L in
                           zip(np.concatenate([[0], np.cumsum(seqlens)[:-1]]), seqlens)])
    inp = dict(scores=synth.scores(T, N, 40, 99), seqs=seqs, seqlens=seqlens)
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    assert r["finite"] and r["loss_rel"] < LOSS_RTOL and r["grad_abs"] < GRAD_ATOL
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])
    assert r["loss"][5] == 0.0 and np.all(r["grad"][:, 5, :] == 0.0)
    # L = T + 1: exactly one path => every row's posterior is a single 1 on a move id
    g = r["grad"][:, 1, :] * T
    assert np.allclose(np.sort(g, axis=1)[:, 0], -1.0, atol=1e-5)
    assert np.allclose(np.sort(g, axis=1)[:, 1:], 0.0, atol=1e-6)


def test_single_block_and_batch_not_multiple_of_64(oracle_mod, gpu_device):
    from taiyaki_amd import synth
    for T, N in ((1, 1), (3, 65), (33, 130)):
        sc = synth.scores(T, N, 40, 5 + T)
        r = parity.compare_logz(oracle_mod, sc, gpu_device)
        assert r["finite"] and r["logz_rel"] < LOSS_RTOL and r["grad_abs"] < GRAD_ATOL
        v = parity.compare_viterbi(oracle_mod, sc, gpu_device)
        assert v["path_mismatch"] == 0 and v["tb_mismatch"] == 0 and v["fwd_bit_mismatch"] == 0


def test_logz_shift_and_concatenation_invariants(gpu_device):
    """Size-independent properties at BASELINE size (T=800, N=128): adding a constant c to
    every score adds T*c to logZ and leaves the posterior unchanged; posterior rows are
    distributions; logZ of the reversed-time tensor with flip/flop-consistent layout is not
    required, but logZ(T blocks) >= max path score (Viterbi) and <= that + T*log(40)."""
    from taiyaki_amd import decode, layers, synth
    T, N = 800, 128
    x = torch.from_numpy(synth.scores(T, N, 40, 21)).to(gpu_device)
    lz, g = layers._logz_launch(x, True)
    lz2, g2 = layers._logz_launch(x + 1.5, True)
    np.testing.assert_allclose((lz2 - lz).cpu().numpy(), 1.5 * T, rtol=2e-6)
    np.testing.assert_allclose(g2.cpu().numpy(), g.cpu().numpy(), atol=2e-6)
    np.testing.assert_allclose(g.sum(dim=2).cpu().numpy(), 1.0, atol=1e-5)
    assert float(g.min()) >= 0.0
    fwd, _, path = decode.flipflop_viterbi(x)
    best = fwd[-1].max(dim=1).values
    assert bool((lz >= best - 1e-3).all()) and bool((lz <= best + T * np.log(40.0)).all())
    # the Viterbi path's own score equals the sum of the scores it walks through
    p = path.cpu().numpy()
    xs = x.cpu().numpy()
    frm, to = p[:-1], p[1:]
    idx = np.where(to < 4, to * 8 + frm, 32 + frm)
    walked = np.take_along_axis(xs, idx[:, :, None], axis=2)[:, :, 0].astype(np.float64).sum(axis=0)
    np.testing.assert_allclose(walked, best.cpu().numpy(), rtol=1e-5)


def test_crf_loss_bounded_by_logz(gpu_device):
    """-T*crf_loss = log sum over paths consistent with the sequence <= logZ (all paths):
    the assembled lossvector (bin/train_flipflop.py:172-176) is >= 0 for every read."""
    from taiyaki_amd import ctc, layers, synth
    inp = synth.crf_case(800, 128, 23)
    x = torch.from_numpy(inp["scores"]).to(gpu_device)
    lv = ctc.crf_flipflop_loss(x, torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"]), 1.0)
    lv = lv + layers.flipflop_logpartition(x) / 800.0
    assert bool((lv > 0).all())


@pytest.mark.parametrize("ch", [8, 16, 32])
def test_logz_every_chunk_size(oracle_mod, gpu_device, ch, labenv):
    """The chunk size of the transfer/posterior kernels is picked per problem size;
    force each instantiation (TK_LOGZ_CH) on a tensor with a ragged tail (T % 32 != 0)."""
    from taiyaki_amd import synth
    labenv.setenv("TK_LOGZ_CH", str(ch))
    sc = synth.scores(333, 70, 40, 45)
    r = parity.compare_logz(oracle_mod, sc, gpu_device)
    assert r["finite"] and r["logz_rel"] < LOSS_RTOL and r["grad_abs"] < GRAD_ATOL
    assert r["rowsum_dev"] < 1e-5


@pytest.mark.parametrize("ring", ["0", "1"])
@pytest.mark.parametrize("T,N", [(1500, 448), (3333, 200), (2500, 270)])
def test_logz_transfer_register_and_lds_ring_forms(oracle_mod, gpu_device, T, N, ring, labenv):
    """One wave per chunk, score rows through registers (TK_K1_RING=0) or through the
    global_load_lds ring of three row-sets (=1; the default below 900 chunks): ragged last
    chunk (T % 16 != 0), a partial last column (N % 64 != 0), odd and even row counts."""
    from taiyaki_amd import synth
    labenv.setenv("TK_K1_RING", ring)
    sc = synth.scores(T, N, 40, 1000 + T + N)
    r = parity.compare_logz(oracle_mod, sc, gpu_device)
    assert r["finite"] and r["logz_rel"] < LOSS_RTOL and r["grad_abs"] < GRAD_ATOL
    assert r["rowsum_dev"] < 1e-5 and r["nograd_same"] == 0.0


def test_crf_reads_do_not_depend_on_their_batch(gpu_device):
    """Every read of a ragged batch -- empty reads in the middle, single-base reads, one read as
    long as the block allows -- gives bit for bit the loss and gradient it gives alone IN A LAUNCH OF THE SAME SHAPE
    (cells per lane, block length and frame slope follow the batch's longest read -- round 5: a batch with a narrow
    band takes shorter blocks and steeper frames --, so the single read is launched with the batch's bound).  (The
    oracle cannot be asked: the reference's move-index layout gives a read L - 1 slots, minus one
    for an empty read, so an empty read in the middle makes its neighbours' slots overlap.)"""
    from taiyaki_amd import synth
    T, N = 40, 70
    rng = np.random.RandomState(5)
    seqlens = rng.randint(0, 30, size=N).astype(np.int32)
    seqlens[[3, 4, 17, 40, 69]] = 0
    seqlens[[5, 41]] = 1
    seqlens[10] = 36
    inp = synth.crf_case(T, N, 91, seqlens=seqlens)
    loss, grad = parity.run_crf(inp, 1.0, gpu_device)
    assert np.isfinite(loss).all() and np.isfinite(grad).all()
    off = np.concatenate([[0], np.cumsum(seqlens)])
    for n in (2, 3, 5, 9, 10, 16, 17, 18, 39, 40, 41, 68, 69):
        one = dict(scores=np.ascontiguousarray(inp["scores"][:, n:n + 1]), seqs=inp["seqs"][off[n]:off[n + 1]],
                   seqlens=seqlens[n:n + 1])
        l1, g1 = parity.run_crf(one, 1.0, gpu_device, max_seqlen=int(seqlens.max()))
        assert np.array_equal(l1[0], loss[n]) and np.array_equal(g1[:, 0], grad[:, n]), n
        if seqlens[n] == 0:
            assert loss[n] == 0.0 and not grad[:, n].any()


def test_parity_on_saturated_network_outputs(oracle_mod, gpu_device):
    """Scores shaped like GlobalNormFlipFlop's output (5 tanh(y), layers.py:1402-1411) with a wide
    pre-activation: most entries saturate at exactly +-5, so equal scores -- and exact ties in the
    Viterbi recursion -- are everywhere.  All three operators against the oracle; the path must
    still be the reference's (first index wins)."""
    from taiyaki_amd import synth
    T, N = 300, 70
    u1 = synth.uniform01(71, 1, T * N * 40).astype(np.float64)
    u2 = synth.uniform01(71, 2, T * N * 40).astype(np.float64)
    y = np.sqrt(-2.0 * np.log(np.maximum(u1, 2.0 ** -24))) * np.cos(2 * np.pi * u2) * 20.0
    sc = (5.0 * np.tanh(y)).astype(np.float32).reshape(T, N, 40)
    assert (np.abs(sc) == 5.0).mean() > 0.3
    r = parity.compare_logz(oracle_mod, sc, gpu_device)
    assert r["finite"] and r["logz_rel"] < LOSS_RTOL and r["grad_abs"] < GRAD_ATOL
    v = parity.compare_viterbi(oracle_mod, sc, gpu_device)
    assert v["path_mismatch"] == 0 and v["tb_mismatch"] == 0 and v["fwd_bit_mismatch"] == 0
    inp = synth.crf_case(T, N, 72)
    inp["scores"] = sc
    rc = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    assert rc["finite"] and rc["loss_rel"] < LOSS_RTOL and rc["grad_abs"] < GRAD_ATOL
    assert parity.crf_grad_ok(rc), (rc["grad_f64_scaled"], rc["grad_scaled_abs"], rc["ref_noise_scaled"])


def test_logz_above_the_streaming_threshold(gpu_device):
    """T=4000 x N=512 (328 MB of scores: the transfer kernel streams with non-temporal loads, two
    workgroups per CU): posteriors are distributions, and the first 256 reads give bit for bit
    what the same reads give as a tensor of their own (row K shape, plain loads) -- the
    arithmetic per read does not depend on how the tensor is moved."""
    import torch
    from taiyaki_amd import layers, synth
    T, N = 4000, 512
    big = torch.empty((T, N, 40), dtype=torch.float32, device=gpu_device)
    for lo in range(0, N, 128):                                 # generated in slabs: less host memory
        big[:, lo:lo + 128] = torch.from_numpy(synth.scores(T, 128, 40, 900 + lo)).to(gpu_device)
    big.requires_grad_(True)
    lz = layers.flipflop_logpartition(big)
    lz.sum().backward()
    g = big.grad
    assert torch.isfinite(lz).all() and torch.isfinite(g).all()
    assert float((g.sum(dim=2) - 1.0).abs().max()) < 1e-5
    sub = big.detach()[:, :256].contiguous().requires_grad_(True)
    lz2 = layers.flipflop_logpartition(sub)
    lz2.sum().backward()
    assert torch.equal(lz[:256], lz2) and torch.equal(g[:, :256], sub.grad)


def test_logz_streaming_transfer_kernel_is_the_same_arithmetic(oracle_mod, gpu_device, labenv):
    """Score tensors above 300 MB go through the non-temporal-load instantiation of the transfer
    kernel: force it (TK_K1_NT=1) on a tensor the oracle handles in seconds and require the very
    same bits as the plain-load form, and parity with the oracle."""
    from taiyaki_amd import synth
    sc = synth.scores(2000, 330, 40, 4242)
    labenv.setenv("TK_K1_RING", "0")
    labenv.setenv("TK_K1_NT", "0")
    lz0, g0 = parity.run_logz(sc, gpu_device)
    labenv.setenv("TK_K1_NT", "1")
    r = parity.compare_logz(oracle_mod, sc, gpu_device)
    assert r["finite"] and r["logz_rel"] < LOSS_RTOL and r["grad_abs"] < GRAD_ATOL
    assert np.array_equal(r["logz"], lz0) and np.array_equal(r["grad"], g0)


@pytest.mark.parametrize("mode_mb", ["0", "6144"])
@pytest.mark.parametrize("name", ["t7n2_len1", "t50n3_zero_last", "t200n8", "t130n5_long", "t300n3_wide"])
def test_crf_both_gradient_modes(oracle_mod, gpu_device, name, mode_mb, labenv):
    """The gradient path has two implementations: the linear-domain banded sweep + recomputing
    gradient pass (csrc/crf_band.hip) and the log-domain checkpoint + recompute kernel (one launch)
    for batches whose checkpoint columns exceed the workspace cap -- and for the reads the first
    one disowns.  TK_CRF_LATTICE_MB=0 forces the second; both must match the oracle."""
    labenv.setenv("TK_CRF_LATTICE_MB", mode_mb)
    inp = cases.crf_inputs(cases.CRF_SMALL[name])
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    assert r["finite"]
    assert r["loss_rel"] < LOSS_RTOL, r["loss_rel"]
    assert r["grad_abs"] < GRAD_ATOL, r["grad_abs"]
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])
    assert r["rowsum_dev"] < 1e-4


@pytest.mark.parametrize("R", ["1", "2", "4"])
def test_crf_band_shapes_against_oracle(oracle_mod, gpu_device, R, labenv):
    """Band mode at every cells-per-lane setting: chunk counts from 1 to several, a last chunk
    with one or two live cells, L = T + 1, T not a multiple of the 8-step time block, an empty
    read in the middle of the batch."""
    from taiyaki_amd import synth
    labenv.setenv("TK_CRF_MODE", "band")
    labenv.setenv("TK_CRF_BAND_R", R)
    PW = 64 * int(R)
    for T, Ls in ((203, [1, PW, PW + 1, PW + 2, 2 * PW, 0, 150, 204, 97]),
                  (61, [62, 30, 5, 61]),
                  (520, [3 * PW + 3 if 3 * PW + 3 <= 521 else 500, 2 * PW + 1, 333])):
        Ls = [min(L, T + 1) for L in Ls]
        inp = synth.crf_case(T, len(Ls), 77 + T, seqlens=np.array(Ls, dtype=np.int32))
        # (the reference cannot index an empty read that is not last: compare the others singly)
        off = np.concatenate([[0], np.cumsum(Ls)])
        loss, grad = parity.run_crf(inp, 1.0, gpu_device)
        for n, L in enumerate(Ls):
            if L == 0:
                assert loss[n] == 0.0 and np.all(grad[:, n] == 0.0)
                continue
            one = dict(scores=np.ascontiguousarray(inp["scores"][:, n:n + 1]), seqs=inp["seqs"][off[n]:off[n + 1]],
                       seqlens=np.array([L], dtype=np.int32))
            oloss, ograd = parity.oracle_crf(oracle_mod, one, 1.0)
            # (a loss that is itself ~0 is a cancelled sum: bound its absolute error instead)
            assert (parity.rel_err(loss[n:n + 1], oloss) < LOSS_RTOL
                    or parity.abs_err(loss[n:n + 1], oloss) < 2e-6), (T, L, loss[n], oloss)
            assert parity.abs_err(grad[:, n:n + 1], ograd) * T < GRAD_T_ATOL, (T, L)


def _crf_alone(inp, n, L, off):
    return dict(scores=np.ascontiguousarray(inp["scores"][:, n:n + 1]), seqs=inp["seqs"][off[n]:off[n + 1]],
                seqlens=np.array([L], dtype=np.int32))


@pytest.mark.parametrize("R", ["1", "4"])
def test_crf_linear_band_path_disowns_reads_and_the_log_domain_kernel_redoes_them(oracle_mod, gpu_device, R,
                                                                                  labenv):
    """Round 3: the band path works in the LINEAR domain (per-cell power-of-two frames) and is
    exact or says so.  One batch holds reads it keeps (wide bands), reads it must disown (bands
    a few cells wide lose their front to the frames' flush; L = T + 1 is one forced path) and an
    empty read.  (a) as shipped every read matches the oracle; (b) with the fallback launch
    suppressed (TK_CRF_NO_FALLBACK=1) and the outputs poisoned, the kept reads are already right
    and the disowned ones are NOT computed -- nobody returns a wrong number."""
    import torch
    from taiyaki_amd import ctc, synth
    labenv.setenv("TK_CRF_MODE", "band")
    labenv.setenv("TK_CRF_BAND_R", R)
    T, Ls = 400, [200, 390, 401, 150, 399, 266, 1, 0]
    inp = synth.crf_case(T, len(Ls), 5, seqlens=np.array(Ls, dtype=np.int32))
    off = np.concatenate([[0], np.cumsum(Ls)])
    x = torch.from_numpy(inp["scores"]).to(gpu_device)
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])

    def run():
        junk = [torch.full_like(x, float("nan")), torch.full((len(Ls),), float("nan"), device=gpu_device)]
        del junk                        # the caching allocator hands these blocks out for the outputs
        c, g = ctc._run(x, seqs, sl, 1.0, 1.0, 1.0, 40, True)
        torch.cuda.synchronize()
        return c.cpu().numpy(), g.cpu().numpy()

    cost, grad = run()
    labenv.setenv("TK_CRF_NO_FALLBACK", "1")
    cost_nf, grad_nf = run()
    kept = []
    for n, L in enumerate(Ls):
        if L == 0:
            assert cost[n] == 0.0 and np.all(grad[:, n] == 0.0)
            continue
        oloss, ograd = parity.oracle_crf(oracle_mod, _crf_alone(inp, n, L, off), 1.0)
        # (a loss that is itself ~0 is a cancelled sum: bound its absolute error instead)
        assert (parity.rel_err(cost[n:n + 1], oloss) < LOSS_RTOL
                or parity.abs_err(cost[n:n + 1], oloss) < 2e-6), (L, cost[n], oloss)
        assert parity.abs_err(grad[:, n:n + 1], ograd) * grad.shape[0] < GRAD_T_ATOL, L
        own = np.isfinite(cost_nf[n]) and np.isfinite(grad_nf[:, n]).all()
        if own:
            kept.append(L)
            assert cost_nf[n] == cost[n] and np.array_equal(grad_nf[:, n], grad[:, n])
    # wide bands stay on the linear path, the forced path (L = T + 1) and the 2-cell band do not
    assert 200 in kept and 150 in kept and 266 in kept, kept
    assert 401 not in kept and 399 not in kept, kept


@pytest.mark.parametrize("bursty", [False, True])
def test_crf_linear_band_path_keeps_confident_reads(oracle_mod, gpu_device, bursty, labenv):
    """Scores of a trained network (synth.confident_scores: the alignment's transition at +4, every
    other at -3) put the whole posterior on one path; a strand that starts in a burst runs that path
    along the band's diagonal edge (position = block + 1), where the move into the first cell of the
    next 64-cell chunk is the row's only instance with mass.  The linear path alone
    (TK_CRF_NO_FALLBACK=1, outputs poisoned) must own every such read and match the oracle."""
    import torch
    from taiyaki_amd import ctc, synth
    labenv.setenv("TK_CRF_MODE", "band")
    labenv.setenv("TK_CRF_NO_FALLBACK", "1")
    T, Ls = 400, [250, 130, 64, 65, 66, 200, 301, 129, 193, 180, 90, 257]
    inp = synth.crf_case(T, len(Ls), 11, seqlens=np.array(Ls, dtype=np.int32))
    synth.confident_scores(inp, 3, bursty=bursty)
    if bursty:
        # reads 0 .. 3 open with one move per block for as long as they have labels: the diagonal
        S = inp["scores"].shape[2]
        off0 = np.concatenate([[0], np.cumsum(Ls)])
        rng = np.random.RandomState(4)
        for n in range(4):
            codes = inp["seqs"][off0[n]:off0[n + 1]].astype(int)
            sc = (-3.0 + rng.uniform(-1, 1, size=(T, S))).astype(np.float32)
            for t in range(T):
                p = min(t, Ls[n] - 1)
                tid = codes[p] + min(codes[p + 1] if t < Ls[n] - 1 else codes[p], 4) * 8
                sc[t, tid] = 4.0 + rng.uniform(-1, 1)
            inp["scores"][:, n, :] = sc
    off = np.concatenate([[0], np.cumsum(Ls)])
    x = torch.from_numpy(inp["scores"]).to(gpu_device)
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    junk = [torch.full_like(x, float("nan")), torch.full((len(Ls),), float("nan"), device=gpu_device)]
    del junk
    c, g = ctc._run(x, seqs, sl, 1.0, 1.0, 1.0, 40, True)
    torch.cuda.synchronize()
    cost, grad = c.cpu().numpy(), g.cpu().numpy()
    assert np.isfinite(cost).all() and np.isfinite(grad).all(), np.nonzero(~np.isfinite(cost))[0]
    for n, L in enumerate(Ls):
        oloss, ograd = parity.oracle_crf(oracle_mod, _crf_alone(inp, n, L, off), 1.0)
        assert parity.rel_err(cost[n:n + 1], oloss) < LOSS_RTOL, (L, cost[n], oloss)
        assert parity.abs_err(grad[:, n:n + 1], ograd) * grad.shape[0] < GRAD_T_ATOL, L


@pytest.mark.parametrize("case", ["step", "ragged", "r2", "catmod", "catmod_wide", "lastblock", "r4", "bk8"])
def test_crf_weight_feeds_change_no_bit(gpu_device, case, labenv):
    """Round 4: one row-maker wave per sweep workgroup exponentiates every score row once and leaves it in
    an LDS ring; the chunk waves gather their step weights from there (crf_band.hip: band_rowmaker) instead
    of loading, exponentiating and ds_bpermute-gathering the rows themselves.  Same values, same order: costs
    and gradients must agree BIT FOR BIT between the two feeds -- for the train step's shape, ragged /
    degenerate lengths, two and four cells per lane, cat-mod with per-column factors, a last block of three
    rows, a cost-only call and 8-step blocks."""
    import torch
    from taiyaki_amd import ctc, synth
    labenv.setenv("TK_CRF_MODE", "band")
    T, N, lens, mods = {"step": (800, 64, "real", None), "ragged": (200, 7, [90, 150, 201, 30, 195, 64, 65], None),
                        "r2": (1600, 16, "real", None), "catmod": (400, 24, "real", (1, 1, 0, 0)),
                        "catmod_wide": (400, 24, "real", (2, 2, 1, 0)),
                        "lastblock": (803, 9, "real", None), "r4": (2600, 6, [2100, 1300, 2500, 900, 1, 2590], None),
                        "bk8": (800, 32, "real", None)}[case]
    if case == "bk8":
        labenv.setenv("TK_CRF_BK", "8")
        labenv.setenv("TK_CRF_WBIAS", "0")
    seqlens = synth.realistic_seqlens(T, N, 17000, T * 5, 9.0) if lens == "real" else np.array(lens, dtype=np.int32)
    inp = synth.crf_case(T, N, 3, seqlens=seqlens, nmods_per_base=mods)
    extra = ()
    if mods is not None:
        synth.normalise_mod_columns(inp, logit_scale=0.2)
        extra = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"])
    x = torch.from_numpy(inp["scores"]).to(gpu_device)
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    out = {}
    for feed in ("self", "rows"):
        labenv.setenv("TK_CRF_FEED", feed)
        res = []
        for want_grad in (True, False):
            if extra:
                c, g = ctc._run(x, seqs, sl, 1.0, 1.0, 1.0, 40, want_grad, *extra)
            else:
                c, g = ctc._run(x, seqs, sl, 1.0, 1.0, 1.0, x.shape[2], want_grad)
            torch.cuda.synchronize()
            res += [c.cpu().numpy()] + ([g.cpu().numpy()] if want_grad else [])
        out[feed] = res
    assert np.isfinite(out["self"][0]).all()
    for a, b in zip(out["self"], out["rows"]):
        assert np.array_equal(a, b)


def test_catmod_column_weights_form_agrees_with_the_general_form(oracle_mod, gpu_device, labenv):
    """Round 3: when the caller passes `mod_col_weights` (the Python operator always does: modfact is
    mod_cat_weights gathered by column) a cat-mod move weight exp(sharp s[move] + factor s[mod]) is the
    product of two gathers from a row exponentiated once per wave; without it (arbitrary per-position
    factors: the reference's C prototype) every cell and step takes its own exponential.  Same
    mathematics, different rounding: both must match the oracle, and each other far inside the tolerance."""
    import torch
    from taiyaki_amd import ctc, synth
    labenv.setenv("TK_CRF_MODE", "band")
    T, N = 400, 24
    seqlens = synth.realistic_seqlens(T, N, 17000, T * 5, 9.0)
    inp = synth.crf_case(T, N, 8, seqlens=seqlens, nmods_per_base=(1, 1, 0, 0))
    synth.normalise_mod_columns(inp, logit_scale=0.2)
    x = torch.from_numpy(inp["scores"]).to(gpu_device)
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    extra = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"])
    out = {}
    labenv.delenv("TK_CATMOD_GENERAL", raising=False)
    for general in ("", "1"):
        if general:
            labenv.setenv("TK_CATMOD_GENERAL", "1")
        c, g = ctc._run(x, seqs, sl, 1.0, 1.0, 1.0, 40, True, *extra)
        torch.cuda.synchronize()
        out[general] = (c.cpu().numpy(), g.cpu().numpy())
    oloss, ograd = parity.oracle_crf(oracle_mod, inp, 1.0)
    for c, g in out.values():
        assert np.isfinite(c).all() and np.isfinite(g).all()
        assert parity.rel_err(c, oloss) < LOSS_RTOL and parity.abs_err(g, ograd) < 5e-5
    assert not np.array_equal(out[""][1], out["1"][1])          # (really two code paths)
    assert parity.rel_err(out[""][0], out["1"][0]) < 1e-5 and parity.abs_err(out[""][1], out["1"][1]) < 5e-6


@pytest.mark.parametrize("catmod", [False, True])
def test_index_build_inside_the_launch_changes_no_bit(gpu_device, catmod, labenv):
    """Round 5: the operators hand the flip-flop codes to `tk_crf_flipflop_labels_dev` /
    `tk_flipflop_loss_fused_labels_dev`, whose sweep workgroups form their ids from the codes themselves (the rank
    workgroups leave the index arrays for the launches behind) -- one launch less than
    `tk_flipflop_build_indices_dev` + the entry points that take its arrays (TK_SEPARATE_INDEX_BUILD=1).  Same
    ids, same arithmetic: gradient call, cost-only call and fused loss agree bit for bit, on a ragged batch with an
    empty read, a one-base read and L = T + 1, and on a batch the log-domain kernel takes (sharpening 9)."""
    import torch
    from taiyaki_amd import ctc, synth
    T = 203
    seqlens = np.array([150, 1, T + 1, 64, 0, 65, 97, 128, 33], dtype=np.int32)
    inp = synth.crf_case(T, len(seqlens), 31, seqlens=seqlens, nmods_per_base=(1, 1, 0, 0) if catmod else None)
    extra = ()
    if catmod:
        synth.normalise_mod_columns(inp, logit_scale=0.2)
        extra = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"])
    x = torch.from_numpy(inp["scores"]).to(gpu_device)
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    # (round 6: the labels entry points also take the batch's BULK length, which picks the block configuration; the entry
    # points that take index arrays do not -- the comparison is between two index builds under ONE configuration, so the
    # lengths carry their maximum and no bulk)
    sl = ctc.set_max_seqlen(sl, int(seqlens.max()))

    def run_all():
        out = []
        for sharp in (1.0, 9.0):
            for want_grad in (True, False):
                c, g = ctc._run(x, seqs, sl, sharp, 1.0 if catmod else sharp, 1.0 / sharp, 40, want_grad, *extra)
                torch.cuda.synchronize()
                out += [c.cpu().numpy()] + ([g.cpu().numpy()] if want_grad else [])
        lv, g, lz = ctc._run_fused(x, seqs, sl, 1.0, True, 1.0, None, *extra)
        torch.cuda.synchronize()
        return out + [lv.cpu().numpy(), g.cpu().numpy(), lz.cpu().numpy()]

    labenv.lib()                        # (the switch is read on the lab build only: both runs there)
    labenv.delenv("TK_SEPARATE_INDEX_BUILD", raising=False)
    inside = run_all()
    labenv.setenv("TK_SEPARATE_INDEX_BUILD", "1")
    separate = run_all()
    assert np.isfinite(inside[0]).all()
    for a, b in zip(inside, separate):
        assert np.array_equal(a, b)


@pytest.mark.parametrize("mods", [(2, 2, 1, 0), (3, 2, 2, 1), (5, 5, 4, 4)])
def test_catmod_rows_wider_than_the_shared_row_image(oracle_mod, gpu_device, mods):
    """Round 4's shared-rows feed keeps 48 columns per exponentiated row in LDS; cat-mod with five or
    more modifications has S = 44 + nmod >= 49 (the C ABI takes up to 62).  Such calls must take the
    per-wave feed (round-4 advisor finding: ids >= 48 gathered from the NEXT row's image, a cost-only call
    then returned a silently wrong cost): gradient call and cost-only call against the oracle, as shipped
    (release library, no switch)."""
    import torch
    from taiyaki_amd import ctc, synth
    T, N = 400, 24
    seqlens = synth.realistic_seqlens(T, N, 17000, T * 5, 9.0)
    inp = synth.crf_case(T, N, 13, seqlens=seqlens, nmods_per_base=mods)
    synth.normalise_mod_columns(inp, logit_scale=0.2)
    assert inp["scores"].shape[2] == 44 + sum(mods) >= 49
    x = torch.from_numpy(inp["scores"]).to(gpu_device)
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    extra = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"])
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    # (more modifications per base = smaller log-softmax values x the weight of 8: reads leave the linear path's
    # range -- 5 of 24 at two modifications per base, 19 and all 24 for the wider alphabets -- and are redone)
    if sum(mods) == 5:
        assert ctc.last_gate_count() <= N // 2, ctc.last_gate_count()
    assert r["finite"] and parity.crf_loss_ok(r), r["loss_rel"]
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])
    # COST-ONLY call (round 5): its forward sweep used to write the cost by itself whenever its score was finite -- the
    # reads above that the gradient call disowns came back silently wrong (costs off by up to 0.19 at (5, 5, 4, 4)).
    # Now both sweeps run and crf_kernel's vote pass believes them only where they agree; the rest is redone.
    c0, _ = ctc._run(x, seqs, sl, 1.0, 1.0, 1.0, 40, False, *extra)
    torch.cuda.synchronize()
    c0 = c0.cpu().numpy()
    assert np.all((np.abs(c0 - r["oloss"]) <= 1e-5 * np.abs(r["oloss"])) | (np.abs(c0 - r["oloss"]) <= 1e-5)), np.abs(c0 - r["oloss"]).max()


@pytest.mark.parametrize("sharp,bk", [(1.3, 8), (1.5, 8), (1.75, 8), (2.0, 4), (2.5, 4), (3.4, 4)])
def test_crf_sharpened_scores_stay_on_the_linear_path(oracle_mod, gpu_device, labenv, sharp, bk):
    """The reference's trainer takes a sharpening schedule (bin/_bin_argparse.py:58-62, applied at
    bin/train_flipflop.py:161-173).  Round 3's linear path overflowed above 1.36 and handed every such
    read to the log-domain kernel; the block length and the weights' bias now follow the factor
    (crf_band_pick_block: 8 steps up to 1.36, biased weights up to 1.76, 4-step blocks up to 3.5), so a
    trained network's sharpened batch keeps every read: parity with the oracle AND a gate count of 0."""
    from taiyaki_amd import _lib, ctc, synth
    labenv.setenv("TK_CRF_MODE", "band")
    T, N = 300, 12
    inp = synth.crf_case(T, N, 9, seqlens=synth.realistic_seqlens(T, N, 5, T * 5, 9.0))
    synth.confident_scores(inp, 11, bursty=False)
    r = parity.compare_crf(oracle_mod, inp, sharp, gpu_device)
    assert _lib.is_strict() and ctc.last_gate_count() == 0
    assert r["finite"]
    assert r["loss_rel"] < LOSS_RTOL, r["loss_rel"]
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])
    # ... and so do freshly initialised scores (|score| <= 1) and iid ones at their full range
    for k, scale in enumerate((0.2, 1.0)):
        inp2 = synth.crf_case(T, N, 19 + k, seqlens=inp["seqlens"])
        inp2["scores"] = (inp2["scores"] * np.float32(scale)).astype(np.float32)
        r2 = parity.compare_crf(oracle_mod, inp2, sharp, gpu_device)
        assert r2["finite"] and r2["loss_rel"] < LOSS_RTOL and parity.crf_grad_ok(r2), (scale, r2["loss_rel"])
        assert ctc.last_gate_count() == 0, (sharp, scale, ctc.last_gate_count())


def test_crf_sharpening_beyond_the_linear_path_goes_to_the_log_domain_kernel(oracle_mod, gpu_device, labenv):
    """sharp = 5 puts weights of 2^(+-36) on a step: no block length holds that; the dispatcher sends
    the call to the log-domain kernel (every read), and the answer is still the oracle's."""
    from taiyaki_amd import synth
    labenv.setenv("TK_CRF_MODE", "band")
    T, N = 300, 6
    inp = synth.crf_case(T, N, 9)
    r = parity.compare_crf(oracle_mod, inp, 5.0, gpu_device)
    assert r["finite"]
    assert r["loss_rel"] < LOSS_RTOL, r["loss_rel"]
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])


@pytest.mark.parametrize("bk,wbias", [("4", "0"), ("8", "0"), ("8", "3"), ("12", "3")])
@pytest.mark.parametrize("mods", [None, (1, 1, 0, 0)])
def test_crf_block_lengths_and_weight_bias_agree_with_the_oracle(oracle_mod, gpu_device, labenv, bk, wbias, mods):
    """Every block length x bias the dispatcher can pick (forced here through the lab switches), plain
    and cat-mod, on lengths around the block and chunk boundaries: T = 1, T below a block, a last block
    of one row, reads of 1 / 64 / 65 / T / T + 1 bases, two cells per lane.  The bias must come back out
    of the scores exactly (costs to 1e-5) and leave the posteriors alone."""
    from taiyaki_amd import synth
    labenv.setenv("TK_CRF_MODE", "band")
    labenv.setenv("TK_CRF_BK", bk)
    labenv.setenv("TK_CRF_WBIAS", wbias)
    for T, Ls in ((1, [1, 2]), (3, [2, 4, 1]), (11, [5, 12, 1]), (13, [13, 7]), (25, [9, 26, 25, 1]),
                  (97, [64, 65, 33, 98, 1]), (300, [129, 257, 64, 200, 301, 0])):
        inp = synth.crf_case(T, len(Ls), 40 + T, seqlens=np.array(Ls, dtype=np.int32), nmods_per_base=mods)
        if mods is not None:
            synth.normalise_mod_columns(inp)
        r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
        assert r["finite"] and parity.crf_loss_ok(r) and r["loss_abs"] < 1e-5, (T, bk, wbias, r["loss_rel"], r["loss_abs"])
        assert parity.crf_grad_ok(r), (T, bk, wbias, r["grad_f64_scaled"], r["ref_noise_scaled"])
    # two cells per lane (reads of 961 .. 1920 bases)
    T = 1500
    inp = synth.crf_case(T, 3, 77, seqlens=np.array([1100, 700, 1300], dtype=np.int32), nmods_per_base=mods)
    if mods is not None:
        synth.normalise_mod_columns(inp)
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    assert r["finite"] and r["loss_rel"] < LOSS_RTOL and parity.crf_grad_ok(r), (bk, wbias, r["loss_rel"])


@pytest.mark.parametrize("form,maxlen", [("plain", 512), ("plain", 513), ("plain", 700), ("catmod", 704), ("catmod", 705), ("catmod", 800),
                                         ("plain", 780), ("plain", 781), ("plain", 900), ("catmod", 992), ("catmod", 993), ("catmod", 1248),
                                         ("catmod", 1249), ("catmod", 1400)])
def test_dispatch_rules_of_round_5_against_the_oracle(oracle_mod, gpu_device, form, maxlen):
    """The RELEASE library's own choices, no lab switch: the plain CRF takes two cells per lane from 513 bases on
    (crf_band_pick_R), cat-mod with per-column factors takes 12-step blocks and the weights' bias from 705 bases on
    (crf_band_pick_block); a batch with narrow bands -- a read beyond 0.78 T, cat-mod 0.62 T -- takes 8-step blocks, bias 3 and
    frames of slope 11, cat-mod beyond 0.78 T 4-step blocks and slope 20 (T = 1000 plain, 1600 cat-mod: 780 / 781, 992 / 993,
    1248 / 1249).  Batches whose longest read sits on either side of each threshold, through the operator
    (workspace from the library's query: it must hold whichever layout the call picks), against the oracle -- and
    every read stays on the linear path."""
    from taiyaki_amd import ctc, synth
    # (cat-mod under iid scores and random labels disowns a read or two of such a batch once L > 0.7 T -- its bands lose
    # mass to the flush where the plain CRF's do from 0.88 T on; the log-domain kernel makes them right, but this test is
    # about the linear path's two forms, so cat-mod gets the reference's usual L ~ T / 2)
    T = 1000 if form == "plain" else 1600
    Ls = np.array([maxlen, 64, maxlen - 1, 333, 129, 1, maxlen - 70], dtype=np.int32)
    mods = (1, 1, 0, 0) if form == "catmod" else None
    inp = synth.crf_case(T, len(Ls), 500 + maxlen, seqlens=Ls, nmods_per_base=mods)
    if mods is not None:
        synth.normalise_mod_columns(inp)
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    # (the loss against the fp32 oracle -- or, where that reference is itself 1e-5 off at T = 1600 on a narrow band, against
    # the float64 witness)
    assert r["finite"] and (parity.crf_loss_ok(r) or r["loss_f64_rel"] < 1e-5), (form, maxlen, r["loss_rel"], r["loss_abs"], r["loss_f64_rel"])
    assert parity.crf_grad_ok(r), (form, maxlen, r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])
    assert ctc.last_gate_count() == 0, (form, maxlen, ctc.last_gate_count())


def test_crf_disowned_reads_are_counted_and_redone_in_shared_slots(oracle_mod, gpu_device, labenv):
    """A batch in which MOST reads are bands a few cells wide under iid scores (the linear path disowns
    those): the log-domain kernel behind it redoes them in an eighth of the batch's worth of checkpoint
    slots, several reads per workgroup one after the other -- every read is the oracle's --, the status
    word's count says how many there were (`ctc.last_gate_count`), and the trainer's watch turns that
    into a warning."""
    import warnings
    from taiyaki_amd import _lib, ctc, synth, train
    labenv.setenv("TK_CRF_MODE", "band")
    T, N = 200, 40
    Ls = np.array([T + 1 - (k % 6) if k % 4 else 90 for k in range(N)], dtype=np.int32)   # 30 narrow bands, 10 ordinary reads
    inp = synth.crf_case(T, N, 5, seqlens=Ls)
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    assert r["finite"] and parity.crf_loss_ok(r), (r["loss_rel"], r["loss_abs"])
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])
    # round 6: the retry launch sweeps the disowned reads again, alone and at 4 steps / slope 20, in the 4 slots 40 reads
    # get (its workgroups loop) -- it keeps most of them; what it disowns too is redone in the log domain
    retried, redone = ctc.last_retry_count(), ctc.last_gate_count()
    assert 10 <= retried <= 30 and redone < retried, (retried, redone)
    # ... and without the retry launch (lab switch): all of them go to the log-domain kernel
    labenv.setenv("TK_CRF_NO_RETRY", "1")
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    assert r["finite"] and parity.crf_loss_ok(r) and parity.crf_grad_ok(r), (r["loss_rel"], r["grad_f64_scaled"])
    gated = ctc.last_gate_count()
    assert 10 <= gated <= 30 and gated == retried and ctc.last_retry_count() == 0, (gated, retried)    # (more than the 5 slots 40 reads get: workgroups looped)
    # non-strict mode: the count accumulates in the deferred word until somebody looks
    _lib.set_strict(False)
    try:
        before = _lib.gated_total()
        parity.run_crf(inp, 1.0, gpu_device)
        parity.run_crf(inp, 1.0, gpu_device)
        assert _lib.take_gate_count() == 2 * gated and _lib.gated_total() == before + 2 * gated
        watch = train.GateWatch(every=2, fraction=0.01)
        parity.run_crf(inp, 1.0, gpu_device)
        watch.note(N)
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            parity.run_crf(inp, 1.0, gpu_device)
            watch.note(N)
        assert any("redone by the log-domain kernel" in str(w.message) for w in seen), [str(w.message) for w in seen]
        assert abs(watch.last_fraction - gated / N) < 1e-6
        _lib.raise_if_nonfinite()
    finally:
        _lib.set_strict(True)


@pytest.mark.parametrize("catmod", [False, True])
def test_tail_launch_paths_cost_only_and_fused(oracle_mod, gpu_device, catmod):
    """Round 6: the tail launch behind the gradient pass (crf_band_tail_kernel) on a batch of ordinary reads with a few bands a
    few cells wide among them -- the fast configuration disowns those, the retry keeps most, the log domain takes the rest.  The three
    forms a caller can reach it by: a gradient call, a COST-ONLY call (the batch's launch leaves every read pending; the tail launch
    compares the sweeps, writes the costs and retries where they disagree) and the FUSED loss (kernel B's gradient is folded into
    the rows the retry's gradient pass writes, too) -- every read is the oracle's."""
    import torch
    from taiyaki_amd import ctc, synth
    T, N = 200, 24
    Ls = np.array([T - 2 - (k % 5) if k % 6 == 0 else 70 + 3 * k for k in range(N)], dtype=np.int32)    # 4 narrow bands among 20 ordinary reads
    inp = synth.crf_case(T, N, 7, seqlens=Ls, nmods_per_base=(1, 1, 0, 0) if catmod else None)
    if catmod:
        synth.normalise_mod_columns(inp, logit_scale=0.2)
    # (the lengths carry their maximum and NO bulk length -- what a pipeline that keeps them on the device hands over: the batch then
    # runs the fast configuration whatever its long reads; with the bulk known, 4 long reads of 24 would move it to the narrow-band one)
    mx = int(Ls.max())
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device, max_seqlen=mx)
    retried, redone = ctc.last_retry_count(), ctc.last_gate_count()
    assert r["finite"] and parity.crf_loss_ok(r) and parity.crf_grad_ok(r), (r["loss_rel"], r["grad_f64_scaled"], r["ref_noise_scaled"])
    assert 1 <= retried <= 4 and redone <= retried, (retried, redone)
    # cost only
    c0, _ = parity.run_crf(inp, 1.0, gpu_device, want_grad=False, max_seqlen=mx)
    assert ctc.last_retry_count() >= 1 and ctc.last_gate_count() <= ctc.last_retry_count()
    assert np.all((np.abs(c0 - r["oloss"]) <= 1e-5 * np.abs(r["oloss"])) | (np.abs(c0 - r["oloss"]) <= 2e-6)), np.abs(c0 - r["oloss"]).max()
    # the fused loss: (A) + logZ / T with one gradient tensor
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    extra = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"]) if catmod else ()
    lv = ctc.flipflop_loss(x, torch.from_numpy(inp["seqs"]), ctc.set_max_seqlen(torch.from_numpy(inp["seqlens"]), mx), 1.0, *extra)
    lv.sum().backward()
    assert ctc.last_retry_count() >= 1
    sc40 = np.ascontiguousarray(inp["scores"][:, :, :40])
    olz, olgrad = oracle_mod.flipflop_logz_grad(sc40)
    np.testing.assert_allclose(lv.detach().cpu().numpy(), r["oloss"] + olz / T, rtol=1e-5, atol=2e-6)
    want = r["ograd"].copy()
    want[:, :, :40] += olgrad / T
    ps = parity.posterior_scale(inp) * T
    assert np.abs((x.grad.cpu().numpy() - want) * ps).max() < parity.GRAD_T_ATOL + 2.5 * r["ref_noise_scaled"]


@pytest.mark.parametrize("catmod", [False, True])
def test_tail_launch_retry_with_its_own_cells_per_lane(oracle_mod, gpu_device, catmod):
    """The retry's layout has its own cells per lane (crf_band_retry_R: the smallest that leaves 2 W <= 16 waves, so that the tail
    launch's workgroup runs both sweeps at once) -- at 744 bases the batch's launch runs cat-mod at one cell per lane (12 chunk waves)
    and the retry at two (6 + 6).  Long reads among ordinary ones at T 800, lengths without a bulk: retried, kept, the oracle's."""
    from taiyaki_amd import ctc, synth
    T, N = 800, 10
    Ls = np.array([744, 440, 743, 401, 470, 742, 433, 500, 741, 420], dtype=np.int32)
    inp = synth.crf_case(T, N, 21, seqlens=Ls, nmods_per_base=(1, 1, 0, 0) if catmod else None)
    if catmod:
        synth.normalise_mod_columns(inp, logit_scale=0.2)
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device, max_seqlen=int(Ls.max()))
    retried, redone = ctc.last_retry_count(), ctc.last_gate_count()
    assert r["finite"] and parity.crf_loss_ok(r) and parity.crf_grad_ok(r), (r["loss_rel"], r["grad_f64_scaled"], r["ref_noise_scaled"])
    assert 1 <= retried <= 4 and redone == 0, (retried, redone)


def test_crf_log_probability_inputs(oracle_mod, gpu_device, labenv):
    """Scores that are log-probabilities (all <= 0, a log-softmax over the 40 transitions: what
    test_ctc_loss.py feeds the reference) shrink every cell by ~2^-5 per step: inside the range of
    the linear path's frames or not, the result is the oracle's."""
    from taiyaki_amd import synth
    labenv.setenv("TK_CRF_MODE", "band")
    T, N = 250, 5
    inp = synth.crf_case(T, N, 21)
    sc = inp["scores"].astype(np.float64)
    sc = sc - np.log(np.exp(sc).sum(axis=2, keepdims=True))
    inp["scores"] = sc.astype(np.float32)
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    assert r["finite"]
    assert r["loss_rel"] < LOSS_RTOL, r["loss_rel"]
    assert r["grad_abs"] < GRAD_ATOL, r["grad_abs"]
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])


@pytest.mark.parametrize("R", ["1", "2", "4"])
def test_crf_band_does_not_read_what_it_did_not_write(gpu_device, R, labenv):
    """The gradient pass reads only the checkpoint columns and boundary cells the sweeps stored, and
    every store lands whole: the same batch must give the same bits whether the workspace it is
    handed was full of NaN or of zeros (a 16-byte column store whose data registers the next
    instruction overwrote once replaced one dword of a column by that instruction's result --
    only visible this way)."""
    import torch
    from taiyaki_amd import ctc, synth
    labenv.setenv("TK_CRF_MODE", "band")
    labenv.setenv("TK_CRF_BAND_R", R)
    T, N = 800, 96
    seqlens = synth.realistic_seqlens(T, N, 17000, 4000, 9.0)
    inp = synth.crf_case(T, N, 1, seqlens=seqlens)
    x = torch.from_numpy(inp["scores"]).to(gpu_device)
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    outs = []
    for fill in (float("nan"), 0.0, 1e30, float("nan")):
        junk = torch.full((160 * 1024 * 1024,), fill, device=gpu_device)
        del junk                        # back to the caching allocator: the next workspace reuses it
        c, g = ctc._run(x, seqs, sl, 1.0, 1.0, 1.0, 40, True)
        outs.append((c.clone(), g.clone()))
    for c, g in outs[1:]:
        assert torch.equal(c, outs[0][0]) and torch.equal(g, outs[0][1])
    assert bool(torch.isfinite(outs[0][1]).all())


@pytest.mark.parametrize("shape", [(4000, 256), (800, 128), (333, 70)])
def test_logz_and_crf_are_bitwise_reproducible(gpu_device, shape):
    """No atomics anywhere: repeated launches on the same input must agree bit for bit (this
    is what exposes an LDS race -- a chain slot shared with another wave's transpose buffer
    once made 1 run in 3 differ in a single read)."""
    import torch
    from taiyaki_amd import ctc, layers, synth
    T, N = shape
    inp = synth.crf_case(T, N, 3)
    x = torch.from_numpy(inp["scores"]).to(gpu_device)
    seqs, seqlens = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    lz0, g0 = layers._logz_launch(x, True)
    c0, cg0 = ctc._run(x, seqs, seqlens, 1.0, 1.0, 1.0, 40, True)
    for _ in range(8):
        lz, g = layers._logz_launch(x, True)
        assert torch.equal(lz, lz0) and torch.equal(g, g0)
    for _ in range(3):
        c, cg = ctc._run(x, seqs, seqlens, 1.0, 1.0, 1.0, 40, True)
        assert torch.equal(c, c0) and torch.equal(cg, cg0)


def test_hybrid_graph_trainer_matches_eager(gpu_device):
    """HybridGraphTrainer (forward + loss replayed from a hipGraph, eager backward, AdamW on
    parameter aliases) must train exactly like the eager Trainer.  Runs in a child process:
    a failed capture aborts inside the HIP runtime."""
    import os
    import re
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "hybrid_vs_eager.py")
    pr = subprocess.run([sys.executable, script], capture_output=True, text=True, timeout=600)
    if pr.returncode != 0 and "hybrid-ok" not in pr.stdout:
        pytest.skip("hipGraph capture of the MIOpen LSTM forward is not available here: "
                    + pr.stderr[-300:])
    m = re.search(r"loss_rel=(\S+) param_abs=(\S+)", pr.stdout)
    assert m, pr.stdout
    assert float(m.group(1)) < 1e-4 and float(m.group(2)) < 1e-4, pr.stdout


def test_graph_cache_trainer_follows_the_reference_chunk_length_schedule(gpu_device):
    """bin/train_flipflop.py:554-563 draws a new chunk length (and batch size) every iteration:
    GraphCacheTrainer keeps one captured forward + loss graph per shape (lengths drawn from a
    grid), shares the optimiser state, and must train exactly like the eager Trainer over a
    sequence that revisits three lengths."""
    import os
    import re
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "hybrid_vs_eager.py")
    pr = subprocess.run([sys.executable, script, "cache"], capture_output=True, text=True, timeout=900)
    if pr.returncode != 0 and "hybrid-ok" not in pr.stdout:
        pytest.skip("hipGraph capture of the MIOpen LSTM forward is not available here: " + pr.stderr[-300:])
    m = re.search(r"loss_rel=(\S+) param_abs=(\S+) graphs=(\d+)", pr.stdout)
    assert m, pr.stdout
    assert float(m.group(1)) < 1e-4 and float(m.group(2)) < 1e-4 and int(m.group(3)) == 3, pr.stdout


def test_whole_step_graph_trainer_clips_like_eager(gpu_device):
    """GraphedTrainer (the whole step in one hipGraph, ATen LSTM) with adaptive clipping: the
    clamp kernel is captured with +inf thresholds and must start clamping once the rolling
    statistics (fed around every replay) produce thresholds -- same losses and parameters as the
    eager Trainer with a 3-step window."""
    import os
    import re
    import subprocess
    import sys
    script = os.path.join(os.path.dirname(os.path.abspath(__file__)), "helpers", "hybrid_vs_eager.py")
    pr = subprocess.run([sys.executable, script, "whole"], capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0 and "hybrid-ok" in pr.stdout, (pr.stdout[-500:], pr.stderr[-800:])
    m = re.search(r"loss_rel=(\S+) param_abs=(\S+)", pr.stdout)
    assert m and float(m.group(1)) < 1e-4 and float(m.group(2)) < 1e-4, pr.stdout


@pytest.mark.parametrize("scale,T,N", [(4.0, 600, 70), (8.0, 600, 70),
                                        (1.0, 2100, 320), (3.0, 2100, 320), (8.0, 2100, 320)])
def test_logz_wide_dynamic_range(oracle_mod, gpu_device, scale, T, N):
    """Scores U(-5 scale, 5 scale): per-row ranges up to 80 nats, path weights differing by
    thousands of nats -- the per-row / per-step power-of-two exponents must carry it.  The
    larger shape takes the wave-per-chunk transfer kernel, whose matrices are stored with a
    common row exponent where their rows lie within 2^40 of each other (else per-row exponents)."""
    from taiyaki_amd import synth
    sc = (synth.scores(T, N, 40, 77) * np.float32(scale)).astype(np.float32)
    r = parity.compare_logz(oracle_mod, sc, gpu_device)
    assert r["finite"] and r["logz_rel"] < LOSS_RTOL, r["logz_rel"]
    assert r["grad_abs"] < 5e-5, r["grad_abs"]
    assert r["rowsum_dev"] < 1e-4
    inp = synth.crf_case(600, 70, 78)
    inp["scores"] = (inp["scores"] * np.float32(scale)).astype(np.float32)
    rc = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    assert rc["finite"] and rc["loss_rel"] < LOSS_RTOL, rc["loss_rel"]
    assert rc["grad_abs"] < 5e-5, rc["grad_abs"]
    assert parity.crf_grad_ok(rc), (rc["grad_f64_scaled"], rc["grad_scaled_abs"], rc["ref_noise_scaled"])


def test_bench_contract_with_live_rccl_group(gpu_device):
    """bench.py at toy shapes with a (single-rank) RCCL process group forced on: the hybrid
    hipGraph step must coexist with the collective path and its watchdog thread, and the LAST
    line rank 0 prints must be the contract JSON."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", MASTER_PORT="29547", RANK="0", LOCAL_RANK="0",
               WORLD_SIZE="1", TK_FORCE_PROCESS_GROUP="1")
    pr = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--chunk-len", "400",
                         "--batch", "8", "--size", "32", "--steps", "2", "--warmup", "1",
                         "--full", "--no-cpu-baseline", "--no-rowk"],
                        env=env, capture_output=True, text=True, timeout=900)
    assert pr.returncode == 0, pr.stderr[-800:]
    line = pr.stdout.strip().splitlines()[-1]
    out = json.loads(line)
    for key in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step",
                "higher_is_better", "scaling", "vs_baseline", "dtype", "data", "config", "roofline"):
        assert key in out, key
    assert out["value"] > 0 and out["n_gpus"] == 1 and out["scaling"] == "weak"
    assert {"bound", "achieved", "peak", "unit", "frac", "traffic"} <= set(out["roofline"])


def test_bench_two_ranks_self_launched_on_one_gpu(gpu_device):
    """`python bench.py --gpus 2` from a plain shell: the bench starts both ranks itself
    (torch.distributed.run), they shard the batch, reduce the gradient arena from backward hooks,
    bracket the timed steps with barriers and rank 0 alone prints the contract line with
    n_gpus = 2 and a global batch of two shards.  On this 1-GPU box both ranks drive cuda:0 and the
    reduction goes over gloo (TK_BENCH_SHARE_GPU: RCCL refuses two ranks on one device) -- the
    choreography and every kernel are the real ones, the number is not a scaling measurement."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env["TK_BENCH_SHARE_GPU"] = "1"
    pr = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--chunk-len", "400",
                         "--batch", "8", "--size", "32", "--steps", "3", "--warmup", "1", "--full", "--no-rowk"],
                        env=env, capture_output=True, text=True, timeout=1200)
    assert pr.returncode == 0, (pr.stdout[-400:], pr.stderr[-1200:])
    lines = [ln for ln in pr.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(lines) == 1, lines                        # one JSON line: rank 0's
    out = json.loads(lines[0])
    assert out["n_gpus"] == 2 and out["config"]["global_batch"] == 16 and out["value"] > 0
    assert out["rccl"]["ranks"] == 2 and out["rccl"]["bytes"] > 0
    assert "cpu_baseline" not in out                     # N > 1 lines carry no CPU leg


def test_logz_very_long_chunks(oracle_mod, gpu_device):
    """T = 9000: more 16-row chunks than one LDS image of the middle kernel holds -> the
    launcher falls back to 32-row chunks; T = 21000 exceeds the build and must say so."""
    import torch
    from taiyaki_amd import layers, synth
    sc = synth.scores(9000, 3, 40, 91)
    r = parity.compare_logz(oracle_mod, sc, gpu_device)
    assert r["finite"] and r["logz_rel"] < LOSS_RTOL and r["grad_abs"] < GRAD_ATOL
    big = torch.zeros(21000, 1, 40, device=gpu_device)
    with pytest.raises(RuntimeError):
        layers.flipflop_logpartition(big)


@pytest.mark.parametrize("nbase", [2, 3])
@pytest.mark.parametrize("mode_mb", ["0", "6144"])
def test_crf_other_alphabet_sizes(oracle_mod, gpu_device, nbase, mode_mb, labenv):
    """2- and 3-letter alphabets (S = 12, 24) through both gradient modes; the kernels take
    the transition count at run time, the reference's tests use nbase 2
    (test_ctc_loss.py:80-135)."""
    from taiyaki_amd import synth
    labenv.setenv("TK_CRF_LATTICE_MB", mode_mb)
    inp = synth.crf_case(120, 9, 300 + nbase, nbase=nbase)
    r = parity.compare_crf(oracle_mod, inp, 1.0, gpu_device)
    assert r["finite"] and r["loss_rel"] < LOSS_RTOL, r["loss_rel"]
    assert r["grad_abs"] < GRAD_ATOL, r["grad_abs"]
    assert parity.crf_grad_ok(r), (r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])
    assert r["rowsum_dev"] < 1e-4


def test_config1_mgru_abinitio_lossvector(oracle_mod, gpu_device):
    """BASELINE configs[0] (the reference's own CPU-runnable case): mGru_flipflop size 96
    stride 2 on chunk_len 2000 -> T = 1000, N = 64, realistic sequence lengths.  The network
    output goes through the HIP loss assembly (train_abinitio.py:213-217) and through the CPU
    oracle; the per-read loss vector and the score gradient must agree."""
    from taiyaki_amd import models, synth, train
    torch.manual_seed(3)
    chunk_len, N = 2000, 64
    net = models.mGru_flipflop(size=96, stride=2).to(gpu_device)
    seqlens = synth.realistic_seqlens(1000, N, 9, chunk_len)
    seqs, _ = synth.sequences(seqlens, 9)
    indata = torch.from_numpy(synth.signal_chunks(chunk_len, N, 9)).to(gpu_device)
    outputs = net(indata).detach().requires_grad_(True)
    assert outputs.shape == (1000, N, 40)
    loss, lossvector = train.calculate_loss(lambda _x: outputs, indata, torch.from_numpy(seqs),
                                            torch.from_numpy(seqlens))
    loss.backward()         # (the mean of the loss vector: the kernels write d mean / d outputs directly)
    assert abs(float(loss) - float(lossvector.mean())) < 1e-6
    sc = outputs.detach().cpu().numpy()
    oloss, ograd = oracle_mod.crf_flipflop_loss(sc, seqs, seqlens, 1.0)
    olz, olgrad = oracle_mod.flipflop_logz_grad(sc)
    np.testing.assert_allclose(lossvector.detach().cpu().numpy(), oloss + olz / 1000, rtol=LOSS_RTOL)
    np.testing.assert_allclose(outputs.grad.cpu().numpy(), (ograd + olgrad / 1000) / N, atol=1e-6)


@pytest.mark.parametrize("name", ["t9n3", "t60n4", "t40n2_sharp"])
def test_catmod_producer_to_loss_chain_against_reference_golden(gpu_device, name):
    """cat-mod end to end: the restated `GlobalNormFlipFlopCatMod`
    with the reference's weights -> HIP `cat_mod_flipflop_loss` + HIP logZ / nblk -> backward to
    the layer's input and weights, against lossvector and gradients produced by the genuine
    reference (tests/golden/make_golden_catmod_layer.py)."""
    import torch
    from taiyaki_amd import ctc, layers
    gold = load_golden("catmod_layer.npz")
    g = {k: gold[name + "/" + k] for k in ("W", "b", "x", "y", "seqs", "seqlens", "mod_cats", "mod_cat_weights",
                                          "sharp", "lossvector", "dx", "dW", "db", "can_mods_offsets", "can_nmods")}
    lay = layers.GlobalNormFlipFlopCatMod(g["W"].shape[1], tuple(int(v) for v in g["can_nmods"])).to(gpu_device)
    lay.load_state_dict({"linear.weight": torch.tensor(g["W"]), "linear.bias": torch.tensor(g["b"])}, strict=False)
    x = torch.tensor(g["x"], device=gpu_device, requires_grad=True)
    y = lay(x)
    np.testing.assert_allclose(y.detach().cpu().numpy(), g["y"], rtol=2e-6, atol=2e-6)
    T = y.shape[0]
    lossvector = ctc.cat_mod_flipflop_loss(y, torch.tensor(g["seqs"]), torch.tensor(g["seqlens"]),
                                           torch.tensor(g["mod_cats"]), g["can_mods_offsets"], g["mod_cat_weights"],
                                           float(g["sharp"]))
    ntrans = y.shape[2] - int(g["can_mods_offsets"][-1])
    lossvector = lossvector + layers.flipflop_logpartition(y[:, :, :ntrans]) / float(T)
    np.testing.assert_allclose(lossvector.detach().cpu().numpy(), g["lossvector"], rtol=1e-5)
    lossvector.mean().backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), g["dx"], atol=2e-6, rtol=1e-4)
    np.testing.assert_allclose(lay.linear.weight.grad.cpu().numpy(), g["dW"], atol=2e-6, rtol=1e-4)
    np.testing.assert_allclose(lay.linear.bias.grad.cpu().numpy(), g["db"], atol=2e-6, rtol=1e-4)


def test_catmod_model_train_step_on_gpu(oracle_mod, gpu_device):
    """configs[3]: one `calculate_loss` + backward + optimiser step of `mLstm_cat_mod_flipflop`
    through the HIP cat-mod loss; lossvector and d loss / d outputs checked against the oracle
    on the network's own outputs (bin/train_flipflop.py:161-182)."""
    import torch
    from taiyaki_amd import models, parallel, synth, train
    torch.manual_seed(3)
    chunk_len, stride, nbatch = 600, 5, 6
    T = chunk_len // stride
    net = models.mLstm_cat_mod_flipflop(size=32, stride=stride).to(gpu_device)
    seqlens = synth.realistic_seqlens(T, nbatch, 4, chunk_len, 9.0)
    seqs, bases = synth.sequences(seqlens, 4)
    mods = synth.mod_cats(bases, 4, (1, 1, 0, 0))
    cmo = synth.can_mods_offsets((1, 1, 0, 0))
    mcw = np.full(6, 8.0, dtype=np.float32)
    indata = torch.from_numpy(synth.signal_chunks(chunk_len, nbatch, 4)).to(gpu_device)
    batch = dict(indata=indata, seqs=torch.from_numpy(seqs), seqlens=torch.from_numpy(seqlens),
                 mod_cats=torch.from_numpy(mods), can_mods_offsets=cmo, mod_cat_weights=mcw)
    outputs = net(indata).detach().requires_grad_()
    from taiyaki_amd import ctc, layers
    lv = ctc.cat_mod_flipflop_loss(outputs, batch["seqs"], batch["seqlens"], batch["mod_cats"], cmo, mcw, 1.0)
    lv = lv + layers.flipflop_logpartition(outputs[:, :, :40]) / float(T)
    lv.mean().backward()
    sc = outputs.detach().cpu().numpy()
    oloss, ograd = oracle_mod.cat_mod_flipflop_loss(sc, seqs, seqlens, mods, cmo, mcw, 1.0)
    olz, olgrad = oracle_mod.flipflop_logz_grad(np.ascontiguousarray(sc[:, :, :40]))
    np.testing.assert_allclose(lv.detach().cpu().numpy(), oloss + olz / T, rtol=1e-5)
    want = ograd / nbatch
    want[:, :, :40] += olgrad / (T * nbatch)
    np.testing.assert_allclose(outputs.grad.cpu().numpy(), want, atol=2e-6)
    trainer = train.Trainer(net, parallel.FlatGradArena(net))
    before = [p.detach().clone() for p in net.parameters() if p.requires_grad]
    loss = float(trainer.step(batch).detach())
    assert np.isfinite(loss) and abs(loss - float(lv.mean())) < 1e-4
    assert any(not torch.equal(a, b) for a, b in zip(before, [p for p in net.parameters() if p.requires_grad]))


def test_trainer_accumulates_sub_batches_like_the_reference(gpu_device):
    """bin/train_flipflop.py:153-198: a step over k sub-batches = one backward each, gradients
    divided by k, ONE optimiser step, reported loss = mean of the sub-batch losses."""
    import torch
    from taiyaki_amd import models, parallel, synth, train
    chunk_len, stride, nbatch = 600, 5, 5
    T = chunk_len // stride

    def make(seed):
        seqlens = synth.realistic_seqlens(T, nbatch, seed, chunk_len, 9.0)
        seqs, _ = synth.sequences(seqlens, seed)
        return dict(indata=torch.from_numpy(synth.signal_chunks(chunk_len, nbatch, seed)).to(gpu_device),
                    seqs=torch.from_numpy(seqs), seqlens=torch.from_numpy(seqlens))

    subs = [make(11), make(12), make(13)]
    torch.manual_seed(5)
    net = models.mLstm_flipflop(size=32, stride=stride).to(gpu_device)
    # by hand: mean gradient and mean loss of the three sub-batches
    grads, losses = None, []
    for b in subs:
        net.zero_grad(set_to_none=True)
        loss, _ = train.calculate_loss(net, **b)
        loss.backward()
        g = [p.grad.detach().clone() for p in net.parameters() if p.requires_grad]
        grads = g if grads is None else [a + c for a, c in zip(grads, g)]
        losses.append(float(loss.detach()))
    want = torch.cat([(g / 3.0).reshape(-1) for g in grads])
    arena = parallel.FlatGradArena(net)
    trainer = train.Trainer(net, arena)
    trainer.opt.step = lambda: None                     # keep the accumulated gradient to look at
    loss = trainer.step(subs)
    torch.cuda.synchronize()
    assert abs(float(loss) - float(np.mean(losses))) < 1e-5
    assert torch.allclose(arena.flat, want, rtol=1e-4, atol=1e-6)
    # and a single batch is still a plain step
    one = trainer.step(subs[0])
    assert abs(float(one.detach()) - losses[0]) < 1e-4


# ------------------------------------------------ seeded fuzz sweeps (bounded) ---
@pytest.mark.parametrize("k", list(range(13)) + [13, 14, 16, 19, 22])
def test_fuzz_shapes_seeded_subset(oracle_mod, gpu_device, k):
    """tests/helpers/fuzz_shapes.py under pytest: the thirteen regime-switch shapes of the logZ /
    Viterbi / CRF launchers plus five seeded random ones, every operator against the oracle
    (cat-mod on every third case).  The full 45 + 36 case sweeps remain a script."""
    from tests.helpers import fuzz_shapes
    ok, msg = fuzz_shapes.case(k, np.random.RandomState(100 + k), gpu_device, oracle_mod)
    assert ok, msg


@pytest.mark.parametrize("k", range(8))
def test_fuzz_prep_seeded_subset(gpu_device, k):
    """tests/helpers/fuzz_prep.py under pytest: chunk batches and remapping with random
    parameters, bit for bit against their oracles (eight seeded cases of each)."""
    from tests.helpers import fuzz_prep
    rng = np.random.RandomState(50 + k)
    ok, what = fuzz_prep.chunk_case(k, rng, gpu_device)
    assert ok, what
    ok, what = fuzz_prep.remap_case(k, rng)
    assert ok, what


def test_bad_labels_raise_like_the_reference(gpu_device):
    """The reference asserts that stay / move indices lie in [0, ntrans) (ctc.pyx:127-134) and
    fails loudly on a bad label; here the index builder range-checks flip-flop codes,
    modification categories and sum(seqlen) on the device and the operator raises the same
    `AssertionError` class -- it neither gathers out of range nor returns garbage."""
    import torch
    from taiyaki_amd import ctc, synth
    x = torch.from_numpy(synth.scores(20, 2, 40, 3)).to(gpu_device)
    good = torch.tensor([0, 1, 2, 3, 0, 5])
    assert bool(torch.isfinite(ctc.crf_flipflop_loss(x, good, torch.tensor([3, 3]), 1.0)).all())
    for seqs, seqlens in ((torch.tensor([0, 1, 8, 3, 0, 5]), torch.tensor([3, 3])),      # code 8 >= 2 nbase
                          (torch.tensor([0, -1, 2, 3, 0, 5]), torch.tensor([3, 3])),     # negative code
                          (good, torch.tensor([3, 9]))):                                 # more labels than given
        with pytest.raises(AssertionError, match="labels out of range"):
            ctc.crf_flipflop_loss(x, seqs, seqlens, 1.0)
    xm = torch.from_numpy(synth.scores(20, 2, 46, 4)).to(gpu_device)
    cmo, mcw = synth.can_mods_offsets((1, 1, 0, 0)), np.full(6, 8.0, dtype=np.float32)
    ok_mods = torch.tensor([0, 1, 0, 0, 0, 0])          # A is label 0 ... ; a mod on C (1 mod) is fine
    assert bool(torch.isfinite(ctc.cat_mod_flipflop_loss(xm, good, torch.tensor([3, 3]), ok_mods, cmo, mcw, 1.0)).all())
    bad_mods = torch.tensor([0, 0, 1, 0, 0, 0])         # G has no modification: category 1 is out of range
    with pytest.raises(AssertionError, match="labels out of range"):
        ctc.cat_mod_flipflop_loss(xm, good, torch.tensor([3, 3]), bad_mods, cmo, mcw, 1.0)


@pytest.mark.parametrize("name", list(cases.FULLSIZE))
def test_fused_loss_at_full_size_against_reference_goldens(gpu_device, name):
    """`ctc.flipflop_loss` (tk_flipflop_loss_fused_dev) = crf loss + logZ / nblk in one operator:
    lossvector against the reference's goldens at every BASELINE size, and its single gradient
    tensor against the sum of the two separate operators' gradients."""
    import torch
    from taiyaki_amd import ctc, layers
    spec = cases.FULLSIZE[name]
    inp = parity.fullsize_inputs(name)
    gold = load_golden("fullsize.npz")
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    seqs, seqlens = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    mods = ()
    if "mod_cats" in inp:
        # cat-mod form (round 3): logZ of the canonical columns folded into the cat-mod kernel's writes
        mods = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"])
    lv = ctc.flipflop_loss(x, seqs, seqlens, 1.0, *mods)
    assert (bool(mods) and not spec.get("lsm")) or ctc.last_gate_count() == 0, ctc.last_gate_count()
    np.testing.assert_allclose(lv.detach().cpu().numpy(), gold[name + "/lossvector"], rtol=1e-4)
    lv.sum().backward()
    g = x.grad.clone()
    x.grad = None
    if mods:
        two = (ctc.cat_mod_flipflop_loss(x, seqs, seqlens, *mods, 1.0)
               + layers.flipflop_logpartition(x[:, :, :40]) / float(spec["T"]))
    else:
        two = ctc.crf_flipflop_loss(x, seqs, seqlens, 1.0) + layers.flipflop_logpartition(x) / float(spec["T"])
    two.sum().backward()
    assert float((lv.detach() - two.detach()).abs().max()) < 2e-6 * float(two.detach().abs().max())
    assert float((g - x.grad).abs().max()) < 1e-7


@pytest.mark.parametrize("sharp", [1.0, 2.5])
def test_fused_loss_small_against_oracle(oracle_mod, gpu_device, sharp):
    """Fused operator vs the oracle's (A) + (B) / nblk incl. sharpening (A only), an empty read and
    L = T + 1; its gradient = d A + (d logZ) / nblk."""
    import torch
    from taiyaki_amd import ctc, synth
    T = 57
    seqlens = np.array([20, 1, T + 1, 33, 0], dtype=np.int32)
    inp = synth.crf_case(T, len(seqlens), 12, seqlens=seqlens)
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    lv = ctc.flipflop_loss(x, torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"]), sharp)
    lv.sum().backward()
    oloss, ograd = oracle_mod.crf_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], sharp)
    olz, olgrad = oracle_mod.flipflop_logz_grad(inp["scores"])
    np.testing.assert_allclose(lv.detach().cpu().numpy(), oloss + olz / T, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(x.grad.cpu().numpy(), ograd + olgrad / T, atol=2e-5)


@pytest.mark.parametrize("weighted", [False, True])
def test_mean_loss_operator_hands_over_the_final_gradient(oracle_mod, gpu_device, weighted):
    """ctc.flipflop_mean_loss = calculate_loss's lossvector + its reduction in one operator: the
    kernels scale the gradient per read (1 / nbatch for `lossvector.mean()`, any weight vector
    for the padded-batch mean), so backward returns the saved tensor -- with grad_output = 1 under
    `ctc.backward_unit(loss)` untouched (same storage), otherwise scaled once -- also when the SAME
    graph is differentiated through a scaled loss right after a unit backward."""
    import torch
    from taiyaki_amd import ctc, synth
    T = 120
    # (empty reads last: the oracle -- like the reference -- cannot index one in the middle of a batch)
    seqlens = np.array([50, 1, 100, 77, 30, 0, 0], dtype=np.int32)
    inp = synth.crf_case(T, len(seqlens), 3, seqlens=seqlens)
    N = len(seqlens)
    w_np = None
    if weighted:
        live = (seqlens > 0).astype(np.float32)
        w_np = live / live.sum()
    oloss, ograd = oracle_mod.crf_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], 1.0)
    olz, olgrad = oracle_mod.flipflop_logz_grad(inp["scores"])
    olv = oloss + olz / T
    wts = np.full(N, 1.0 / N, dtype=np.float32) if w_np is None else w_np
    want_loss = float((olv * wts).sum())
    want_grad = (ograd + olgrad / T) * wts[None, :, None]

    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    weights = None if w_np is None else torch.from_numpy(w_np).to(gpu_device)
    loss, lv = ctc.flipflop_mean_loss(x, torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"]), 1.0,
                                      weights)
    assert not lv.requires_grad
    np.testing.assert_allclose(lv.cpu().numpy(), olv, rtol=1e-5, atol=2e-6)
    assert abs(float(loss) - want_loss) < 1e-5 * abs(want_loss) + 2e-6
    ctc.backward_unit(loss, retain_graph=True)
    g1 = x.grad.clone()
    np.testing.assert_allclose(g1.cpu().numpy(), want_grad, atol=2e-5 / N)
    # a grad_output other than 1 is honoured (one scaling pass)
    x.grad = None
    (loss * 3.0).backward()
    np.testing.assert_allclose(x.grad.cpu().numpy(), 3.0 * g1.cpu().numpy(), rtol=1e-6, atol=1e-9)


def test_train_step_has_no_elementwise_pass_between_loss_and_rnn_backward(gpu_device):
    """The trainers differentiate the mean loss with a bare `loss.backward()`: the tensor that
    reaches the network's last layer IS the kernels' output (same storage)."""
    import torch
    from taiyaki_amd import ctc, synth, train
    T, N = 64, 4
    inp = synth.crf_case(T, N, 8)
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    seen = {}
    x.register_hook(lambda g: seen.update(ptr=g.data_ptr()))

    class Net(torch.nn.Module):
        def forward(self, indata):
            return x
    seqlens = torch.from_numpy(inp["seqlens"]).to(gpu_device)
    ctc.set_max_seqlen(seqlens, int(inp["seqlens"].max()))
    loss, _ = train.calculate_loss(Net(), None, torch.from_numpy(inp["seqs"]).to(gpu_device), seqlens)
    fn = loss.grad_fn
    saved = fn.saved_tensors[0].data_ptr()
    ctc.backward_unit(loss)
    assert seen["ptr"] == saved


@pytest.mark.parametrize("sharp", [1.0, 2.5])
def test_fused_catmod_loss_small_against_oracle(oracle_mod, gpu_device, sharp):
    """Cat-mod form of the fused operator vs the oracle's cat-mod loss + logZ(canonical columns) / nblk,
    on mod columns that are log-probabilities (what the producer layer emits: the linear band path
    keeps these reads) -- incl. the reference's sharpening quirk (canonical columns only; the saved
    gradient unscaled, ctc.pyx:265-267, 306-310), an empty read and the weighted mean."""
    import torch
    from taiyaki_amd import ctc, synth
    T = 90
    seqlens = np.array([40, 1, 77, 33, 0], dtype=np.int32)
    inp = synth.normalise_mod_columns(synth.crf_case(T, len(seqlens), 4, seqlens=seqlens, nmods_per_base=(1, 1, 0, 0)),
                                      logit_scale=1.0)
    mods = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"])
    oloss, ograd = oracle_mod.cat_mod_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], inp["mod_cats"],
                                                    inp["can_mods_offsets"], inp["mod_cat_weights"], sharp)
    olz, olgrad = oracle_mod.flipflop_logz_grad(np.ascontiguousarray(inp["scores"][:, :, :40]))
    want_lv = oloss + olz / T
    want_g = ograd.copy()
    want_g[:, :, :40] += olgrad / T
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    lv = ctc.flipflop_loss(x, seqs, sl, sharp, *mods)
    lv.sum().backward()
    np.testing.assert_allclose(lv.detach().cpu().numpy(), want_lv, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(x.grad.cpu().numpy(), want_g, atol=2e-5)
    # ... and as the mean-loss operator with per-read weights
    x.grad = None
    live = (seqlens > 0).astype(np.float32)
    w = torch.from_numpy(live / live.sum()).to(gpu_device)
    loss, lv2 = ctc.flipflop_mean_loss(x, seqs, sl, sharp, w, *mods)
    ctc.backward_unit(loss)
    np.testing.assert_allclose(lv2.cpu().numpy(), want_lv, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(x.grad.cpu().numpy(), want_g * (live / live.sum())[None, :, None], atol=2e-5)


@pytest.fixture
def loss_queues(request):
    """Run a test with the fused loss's one-queue (0) or two-queue (1) form, restoring the library's mode."""
    from taiyaki_amd import _lib
    L = _lib.lib()
    prev = L.tk_flipflop_loss_overlap(request.param)
    yield request.param
    L.tk_flipflop_loss_overlap(prev)


@pytest.mark.parametrize("loss_queues", [0, 1], indirect=True)
@pytest.mark.parametrize("catmod", [False, True])
def test_fused_loss_forms_against_oracle(oracle_mod, gpu_device, loss_queues, catmod):
    """Both forms of the fused operator -- kernel B after kernel A on the caller's queue, adding in place (what a
    captured train step replays), and kernel B on the device's second queue beside A's sweeps, folded into A's
    gradient pass (the default outside a capture, `tk_flipflop_loss_overlap`) -- against the oracle's
    (A) + (B) / nblk on ragged reads (an empty one, a single base, one longer than the chunk), with the weighted
    mean on top; and the library reports the mode it is in."""
    import torch
    from taiyaki_amd import _lib, ctc, synth
    assert _lib.lib().tk_flipflop_loss_overlap(-1) == loss_queues
    T = 133
    seqlens = np.array([60, 1, T + 1, 33, 0, 90, 17], dtype=np.int32)
    if catmod:
        inp = synth.normalise_mod_columns(synth.crf_case(T, len(seqlens), 21, seqlens=seqlens, nmods_per_base=(1, 1, 0, 0)),
                                          logit_scale=1.0)
        mods = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"])
        oloss, ograd = oracle_mod.cat_mod_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], inp["mod_cats"],
                                                        inp["can_mods_offsets"], inp["mod_cat_weights"], 1.0)
    else:
        inp = synth.crf_case(T, len(seqlens), 21, seqlens=seqlens)
        mods = ()
        oloss, ograd = oracle_mod.crf_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], 1.0)
    olz, olgrad = oracle_mod.flipflop_logz_grad(np.ascontiguousarray(inp["scores"][:, :, :40]))
    want_lv = oloss + olz / T
    want_g = ograd.copy()
    want_g[:, :, :40] += olgrad / T
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    for _ in range(3):                                      # (back to back: the fork / join events are reused)
        x.grad = None
        lv = ctc.flipflop_loss(x, seqs, sl, 1.0, *mods)
        lv.sum().backward()
    np.testing.assert_allclose(lv.detach().cpu().numpy(), want_lv, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(x.grad.cpu().numpy(), want_g, atol=2e-5)
    x.grad = None
    w = torch.linspace(0.5, 1.5, len(seqlens)).to(gpu_device)
    loss, lv2 = ctc.flipflop_mean_loss(x, seqs, sl, 1.0, w, *mods)
    ctc.backward_unit(loss)
    np.testing.assert_allclose(lv2.cpu().numpy(), want_lv, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(x.grad.cpu().numpy(), want_g * w.cpu().numpy()[None, :, None], atol=3e-5)


def test_fused_loss_two_queue_form_from_two_host_threads(gpu_device):
    """The side queue and its fork / join events are one per device: two host threads calling the operator on
    streams of their own take turns enqueueing, and each gets the result it gets alone."""
    import threading
    import torch
    from taiyaki_amd import _lib, ctc, synth
    assert _lib.lib().tk_flipflop_loss_overlap(-1) == 1
    cases_ = [synth.crf_case(200, 16, 50 + i) for i in range(2)]
    want = []
    for inp in cases_:
        x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
        lv = ctc.flipflop_loss(x, torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"]), 1.0)
        lv.sum().backward()
        want.append((lv.detach().cpu().numpy(), x.grad.cpu().numpy()))
    got, errors = [None, None], []

    def work(i):
        try:
            inp = cases_[i]
            with torch.cuda.stream(torch.cuda.Stream(device=gpu_device)):
                x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
                for _ in range(20):
                    x.grad = None
                    lv = ctc.flipflop_loss(x, torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"]), 1.0)
                    lv.sum().backward()
                torch.cuda.current_stream().synchronize()
                got[i] = (lv.detach().cpu().numpy(), x.grad.cpu().numpy())
        except Exception as exc:                            # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for i in range(2):
        np.testing.assert_array_equal(got[i][0], want[i][0])
        np.testing.assert_array_equal(got[i][1], want[i][1])



@pytest.mark.parametrize("catmod", [False, True])
def test_crf_alignments_that_cross_chunk_boundaries_inside_a_block_stay_on_the_linear_path(oracle_mod, gpu_device, catmod):
    """The gradient pass decides which 64-cell chunks of a time block carry posterior mass from the cell
    posteriors at the block's FIRST column (crf_band.hip: the column test) -- over the chunk's own cells and the
    last BK cells of the chunk before it, where a path that enters the chunk inside the block sits at that
    column.  Confident scores (one alignment per read, everything else 7 units down) on alignments built to do
    exactly that: runs of one move per block that cross positions 64 and 128 at every offset inside a 12-step
    block, and stalls on a chunk's last cell that end inside a block.  The gradient must match the float64
    witness, and NO read may be handed to the log-domain kernel: a chunk skipped wrongly loses a row's mass,
    the row-total check disowns the read, and the result would still be right -- only the gate count shows it."""
    import torch
    from taiyaki_amd import ctc, synth
    T, L = 204, 150
    N = 26
    seqlens = np.full(N, L, dtype=np.int32)
    inp = synth.crf_case(T, N, 77, seqlens=seqlens, nmods_per_base=(1, 1, 0, 0) if catmod else None)

    def move_times(n):
        if n < 13:
            start = 2 + n                                       # a straight run: position p at block start + p
            return np.arange(start, start + L - 1)
        # stall on the last cell of chunk 0 (position 63), leave it at block 96 + k, k = 0 .. 12
        k = n - 13
        first = np.arange(0, 63)                                # positions 0 -> 63 by block 63
        leave = 96 + k
        rest = np.arange(leave, leave + (L - 1 - 63))
        return np.concatenate([first, rest])

    synth.confident_scores(inp, 5, move_times=move_times)
    margs = ()
    if catmod:
        synth.normalise_mod_columns(inp, logit_scale=0.2)      # (log-probabilities, what the producer layer emits)
        margs = (inp["mod_cats"], inp["can_mods_offsets"], inp["mod_cat_weights"])
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    seqs, sl = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    if catmod:
        lv = ctc.cat_mod_flipflop_loss(x, seqs, sl, torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"], 1.0)
    else:
        lv = ctc.crf_flipflop_loss(x, seqs, sl, 1.0)
    gated = ctc.last_gate_count()
    lv.sum().backward()
    wl, wg = oracle_mod.crf_flipflop_loss_f64(inp["scores"], inp["seqs"], inp["seqlens"], 1.0, *margs)
    np.testing.assert_allclose(lv.detach().cpu().numpy(), wl, rtol=1e-5, atol=2e-6)
    g = x.grad.cpu().numpy().astype(np.float64)
    assert float((np.abs(g - wg) * T * parity.posterior_scale(inp)[None, None, :]).max()) < parity.GRAD_T_ATOL
    # every row of every read carries its whole mass: the canonical columns' posteriors sum to 1
    assert float(np.abs(g[:, :, :40].sum(axis=2) * -T - 1.0).max()) < 1e-4
    assert gated == 0


@pytest.mark.parametrize("T,L", [(1500, 1100), (2600, 2100)])
def test_crf_confident_long_reads_stay_on_the_linear_path(oracle_mod, gpu_device, T, L):
    """The same on reads whose sweeps take two and four cells per lane (sweep chunks of 128 / 256 cells, gradient-pass
    chunks of 64: the frame bases are per SWEEP chunk): straight runs and one stall per read, confident scores --
    gradient against the float64 witness, every row's mass in one transition, no read disowned."""
    import torch
    from taiyaki_amd import ctc, synth
    N = 4
    seqlens = np.full(N, L, dtype=np.int32)
    inp = synth.crf_case(T, N, 78, seqlens=seqlens)

    def move_times(n):
        if n < 2:
            start = 3 + 7 * n
            return np.arange(start, start + L - 1)
        stall_at = 64 * (5 + n) - 1                              # the last cell of a 64-cell chunk
        first = np.arange(0, stall_at)
        leave = stall_at + 101 + n
        return np.concatenate([first, np.arange(leave, leave + (L - 1 - stall_at))])

    synth.confident_scores(inp, 6, move_times=move_times)
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    lv = ctc.crf_flipflop_loss(x, torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"]), 1.0)
    gated = ctc.last_gate_count()
    lv.sum().backward()
    wl, wg = oracle_mod.crf_flipflop_loss_f64(inp["scores"], inp["seqs"], inp["seqlens"], 1.0)
    np.testing.assert_allclose(lv.detach().cpu().numpy(), wl, rtol=1e-5, atol=2e-6)
    assert float(np.abs(x.grad.cpu().numpy().astype(np.float64) - wg).max()) * T < parity.GRAD_T_ATOL
    assert float(np.abs(x.grad.cpu().numpy().sum(axis=2) * -T - 1.0).max()) < 1e-4
    assert gated == 0
