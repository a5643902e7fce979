"""Every alphabet size (NB = 1..4) of the decode side in every kernel form its launchers can choose: logZ and its
posterior (csrc/logz_kernels.hip), the fused loss's accumulate-into-the-gradient posterior store at the small
alphabets, the Viterbi (csrc/viterbi_kernels.hip) and the error probabilities (csrc/qscore_kernels.hip), each launched at
least once and compared with the oracle, with float64, or with a bound derived from the arithmetic.

A case names the form it runs, never only a shape.  The launchers take their choices from small host functions
(logz_plan and viterbi_waves) that the lab build also exports as tk_lab_logz_plan / tk_lab_viterbi_plan; the CPU tests
at the top restate both rules in Python (`logz_rule`, `viterbi_rule`), hold the restatement against the library on a
grid around every threshold, and assert that the tables below reach what they claim to reach.

  logZ forms    (CH, transfer, SUP, tail): CH rows per chunk (8 / 16: 16 where ceil(N / 64) * ceil(T / 16) >= 384; doubled
                while the middle kernel's LDS image exceeds 160 KiB); the transfer kernel by the chunk count
                ceil(N / 64) * ceil(T / CH): cooperative below 640, the global_load_lds ring up to 900, one wave per chunk
                through registers above, its streaming-load instantiation for score tensors above 300 MB; the middle
                kernel's supers of 8 or 16 chunks (16 where there are more than 128 chunks); and whether the posterior
                kernel keeps the hand-off slots of its two chains in a tail behind the waves' transpose buffers
                ((CH / 8 + 2) * 2NB * 64 > 4 * max(64 * S / 4, (CH / 8) * 2NB * 16): (NB, CH) = (1, 8), (1, 16), (2, 16)
                among the release rule's chunk sizes) or inside them (the other five).
  Viterbi forms five waves per read (N <= 640), three (N <= 1536), one (above); each with full outputs or the path only.

LOGZ_SHAPES are the smallest shapes that reach each form with a ragged last chunk and a last column of one or two live
reads.  The last row of the table, (1003, 321), is CH 8 with the ring transfer: 8-row chunks can number up to 766, so the
release rule reaches that instantiation too, and no other test does.

What is compared.  logZ / posterior: the fp32 oracle under the bounds tests/test_gpu_parity.py applies to this operator
(LOSS_RTOL, GRAD_ATOL, row sums within 1e-5 of 1, the launch without a gradient returns the same logZ bit for bit), and a
float64 witness (tests/test_decode_varlen.py::forward_backward) on the first and last live column of every 64-read column
group under the rule of tests/test_lstm_hip.py: error over the tensor's largest entry <= 2 x the fp32 oracle's own + 2e-6.
Viterbi: forward scores, traceback and path bit for bit.  Error probabilities: 1 - p_b / (sum p + 1e-10) in float64; the
numerator is a float32 sum of at most 2NB + 2 non-negative terms, the denominator of at most S, one divide and one
subtract follow: |error| <= (S + 2NB + 4) * 2^-24.  Every GPU case prints its figures and the form the lab plan
reported; profiles/r26_decode_instantiations.txt keeps one run.

What this file found when it was written: nothing.  Every form at every alphabet size agrees with its reference; the
largest figures are in the profile.  That the cases bite was tried once on a scratch build whose two tail slots of
logz_posterior_kernel coincide (the same LDS size and barriers, wrong values): of this file exactly the (1, 8), (1, 16) and
(2, 16) cases failed, and of the suite as it was only test_logz_very_long_chunks, which reaches the tail form at NB 4
through the 32-row fallback."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, decode, synth
from tests import parity, test_lstm_fwd_rows as rows
from tests.test_decode_varlen import forward_backward
from tests.test_gpu_parity import GRAD_ATOL, LOSS_RTOL

NBASES = [1, 2, 3, 4]
COOP, RING, PLAIN, STREAM = 0, 1, 2, 3
TRANSFER = ("cooperative", "ring", "registers", "streaming")

# (T, N): (CH, transfer, SUP) under the release rule, for every NB
LOGZ_SHAPES = {
    (50, 5): (8, COOP, 8),
    (1030, 5): (8, COOP, 16),           # C = 129
    (883, 385): (16, COOP, 8),          # 7 * 56 = 392 >= 384; 392 chunks
    (2051, 130): (16, COOP, 16),        # 3 * 129 = 387
    (1301, 449): (16, RING, 8),         # 8 * 82 = 656 chunks
    (1809, 449): (16, PLAIN, 8),        # 8 * 114 = 912 chunks
    (1003, 321): (8, RING, 8),          # 6 * 63 = 378 < 384; 6 * 126 = 756 chunks of 8 rows
}
STREAM_SHAPE = (1809, 449)              # ... and its streaming-load instantiation, forced: by shape it needs 300 MB
SMALL_SHAPES = [(T, N) for T in (1, 7, 8, 9, 16, 17) for N in (1, 64, 65)]          # all (8, COOP, 8)
TAIL = {(1, 8), (1, 16), (2, 16)}       # (NB, CH) whose posterior kernel keeps its chains behind the buffers
FUSED_SHAPE = (883, 385)                # logz_posterior_kernel<NB, 16, true>

VIT_BATCHES = {11: 5, 641: 3, 1537: 1}  # N: waves per read
VIT_STEPS = {11: [1, 2, 15, 16, 17, 63, 64, 65, 257], 641: [1, 16, 17, 65, 257], 1537: [1, 16, 17, 65, 257]}
VIT_OUTPUTS = ("full", "path")

ERR_BATCHES, ERR_STEPS = [1, 63, 64, 65, 130], [1, 2, 7, 8, 9, 17]


# ---------------------------------------------------------------------------------------------------------------------
# the rules, restated
# ---------------------------------------------------------------------------------------------------------------------
def _nstate(nb):
    return 2 * nb * (nb + 1)


def _middle_lds(nb, C):
    """logz_middle_lds_bytes: [C] chunk matrices, [NSUP] super totals, one of slack, 2 x [NSUP] boundary vectors."""
    nw = 4 * nb * nb + 2 * nb + 2
    sup = 16 if C > 128 else 8
    nsup = -(-C // sup)
    return ((C + nsup + 1) * (nw + (nw & 1)) + 2 * nsup * 8) * 4


def logz_rule(T, N, nb, nbytes):
    """(CH, transfer, SUP, tail) of logz_plan, or None where the middle kernel's LDS image does not fit at CH 32."""
    ncols = -(-N // 64)
    ch = 16 if ncols * -(-T // 16) >= 384 else 8
    while ch < 32 and _middle_lds(nb, -(-T // ch)) > 160 * 1024:
        ch *= 2
    C = -(-T // ch)
    if _middle_lds(nb, C) > 160 * 1024:
        return None
    chunks = ncols * C
    transfer = COOP if chunks < 640 else RING if chunks <= 900 else STREAM if nbytes > (300 << 20) else PLAIN
    tail = (ch // 8 + 2) * 2 * nb * 64 > 4 * max(64 * _nstate(nb) // 4, (ch // 8) * 2 * nb * 16)
    return (ch, transfer, 16 if C > 128 else 8, tail)


def viterbi_rule(N):
    return 5 if N <= 640 else 3 if N <= 1536 else 1


def _score_bytes(T, N, nb):
    return T * N * _nstate(nb) * 4


def _lab_logz_plan(T, N, nb, nbytes=None):
    """The library's own plan at (T, N, nb) under the environment as it stands (tk_lab_logz_plan, the lab library)."""
    was_lab = _lib.is_lab()
    L = _lib.use_lab(True)
    try:
        out = (ctypes.c_size_t * 4)()
        if not L.tk_lab_logz_plan(T, N, nb, _score_bytes(T, N, nb) if nbytes is None else nbytes, out):
            return None
        return (int(out[0]), int(out[1]), int(out[2]), bool(out[3]))
    finally:
        _lib.use_lab(was_lab)


def _lab_viterbi_plan(N):
    was_lab = _lib.is_lab()
    L = _lib.use_lab(True)
    try:
        return int(L.tk_lab_viterbi_plan(N))
    finally:
        _lib.use_lab(was_lab)


def _form(plan):
    return "CH %d, %s, supers of %d, chains %s" % (plan[0], TRANSFER[plan[1]], plan[2], "in the tail" if plan[3] else "in the buffers")


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the rules are the library's, the tables reach what they say
# ---------------------------------------------------------------------------------------------------------------------
def test_logz_rule_is_the_librarys_around_every_threshold():
    L = _lib.use_lab(True)
    try:
        out = (ctypes.c_size_t * 4)()

        def lab(T, N, nb, nbytes):
            return (int(out[0]), int(out[1]), int(out[2]), bool(out[3])) if L.tk_lab_logz_plan(T, N, nb, nbytes, out) else None

        seen = set()
        for nb in NBASES:
            # one to ten column groups, either side of a group's edge; every T up to past 900 chunks of 16 rows in one
            # column group x 2: the 384, 640 and 900 switches and C = 128 fall inside for every N below
            for N in (1, 64, 65, 128, 129, 320, 321, 384, 385, 448, 449, 450, 640, 641):
                for T in range(1, 2400):
                    got, want = lab(T, N, nb, _score_bytes(T, N, nb)), logz_rule(T, N, nb, _score_bytes(T, N, nb))
                    assert got == want, (T, N, nb, got, want)
                    seen.add((nb,) + got)
            # one column group alone reaches the switches only at long T, where the LDS fallback doubles CH
            for N in (1, 64, 65):
                for T in list(range(5000, 15500, 7)) + [6128, 6129, 6144, 6145, 10240, 10241, 14400, 14401, 21000, 40000]:
                    assert lab(T, N, nb, _score_bytes(T, N, nb)) == logz_rule(T, N, nb, _score_bytes(T, N, nb)), (T, N, nb)
            # the streaming-load switch: bytes of the score tensor, strictly above 300 MB, and only past 900 chunks
            for nbytes in (0, 300 << 20, (300 << 20) + 1, 1 << 40):
                for T, N in ((1809, 449), (1301, 449), (50, 5)):
                    assert lab(T, N, nb, nbytes) == logz_rule(T, N, nb, nbytes), (T, N, nb, nbytes)
            assert lab(1809, 449, nb, (300 << 20) + 1)[1] == STREAM and lab(1809, 449, nb, 300 << 20)[1] == PLAIN
        assert lab(50, 5, 0, 4000) is None and lab(50, 5, 5, 4000) is None
        assert logz_rule(40000, 1, 4, 0) is None and logz_rule(40000, 1, 1, 0) is not None
        # the grid itself meets every value of every choice at every alphabet size
        for nb in NBASES:
            for k, values in enumerate(((8, 16), (COOP, RING, PLAIN), (8, 16))):
                assert {s[1 + k] for s in seen if s[0] == nb} == set(values), (nb, k)
            assert {(s[1], s[4]) for s in seen if s[0] == nb} == {(ch, (nb, ch) in TAIL) for ch in (8, 16)}, nb
        assert lab(9000, 3, 4, 0) == (32, COOP, 16, True) == logz_rule(9000, 3, 4, 0)       # the fallback's last step
    finally:
        _lib.use_lab(False)


def test_logz_case_table_reaches_every_form():
    reached = set()
    for nb in NBASES:
        for (T, N), want in LOGZ_SHAPES.items():
            plan = logz_rule(T, N, nb, _score_bytes(T, N, nb))
            assert plan[:3] == want and plan == _lab_logz_plan(T, N, nb), (T, N, nb, plan)
            assert T % plan[0] != 0 and N % 64 in (1, 2, 5), (T, N)       # a ragged last chunk, a last column of few reads
            reached.add((nb,) + plan)
        for T, N in SMALL_SHAPES:
            plan = logz_rule(T, N, nb, _score_bytes(T, N, nb))
            assert plan == (8, COOP, 8, (nb, 8) in TAIL) == _lab_logz_plan(T, N, nb), (T, N, nb, plan)
    # the posterior kernel: every (NB, CH) of the release rule's chunk sizes, the tail form exactly at the three
    assert {(s[0], s[1], s[4]) for s in reached} == {(nb, ch, (nb, ch) in TAIL) for nb in NBASES for ch in (8, 16)}
    assert len(TAIL) == 3 and len({(s[0], s[1]) for s in reached if not s[4]}) == 5
    # ... and every row of the table is needed: a form of its own, at every alphabet size
    for nb in NBASES:
        forms = [s[1:4] for s in reached if s[0] == nb]
        assert sorted(forms) == sorted(LOGZ_SHAPES.values()) and len(set(forms)) == len(LOGZ_SHAPES) == 7, (nb, forms)
        assert {f[1] for f in forms} == {COOP, RING, PLAIN} and {f[0] for f in forms} == {8, 16} == {f[2] for f in forms}
        plan = logz_rule(*STREAM_SHAPE, nb, _score_bytes(*STREAM_SHAPE, nb))
        assert plan[1] == PLAIN                                         # what TK_K1_NT = 1 turns into the streaming form
        assert logz_rule(*FUSED_SHAPE, nb, 0)[0] == 16


def test_viterbi_rule_is_the_librarys_and_the_batches_reach_every_form():
    for N in range(1, 1700):
        assert _lab_viterbi_plan(N) == viterbi_rule(N), N
    assert viterbi_rule(640) == 5 and viterbi_rule(641) == 3 and viterbi_rule(1536) == 3 and viterbi_rule(1537) == 1
    for nb in NBASES:
        reached = {(nb, viterbi_rule(N), out) for N in VIT_BATCHES for out in VIT_OUTPUTS}
        assert reached == {(nb, w, out) for w in (1, 3, 5) for out in ("full", "path")}
    for N, waves in VIT_BATCHES.items():
        assert viterbi_rule(N) == waves == _lab_viterbi_plan(N)
        # around the tile (16), the group and traceback scan (64) and four scans (256)
        assert {1, 16, 17, 65, 257} <= set(VIT_STEPS[N])


def test_witness_columns_are_the_ends_of_every_column_group():
    assert _witness_columns(1) == [0] and _witness_columns(64) == [0, 63] and _witness_columns(65) == [0, 63, 64]
    assert _witness_columns(130) == [0, 63, 64, 127, 128, 129]
    assert len(_witness_columns(449)) == 15 and _witness_columns(449)[-3:] == [384, 447, 448]


def test_witness_agrees_with_the_oracle_at_every_alphabet_size(oracle_mod):
    """forward_backward is generic in the alphabet size; the oracle's posteriors sit ~3e-8 from it at T = 37."""
    for nb in NBASES:
        sc = synth.scores(37, 3, _nstate(nb), 60 + nb)
        olz, ograd = oracle_mod.flipflop_logz_grad(sc)
        ref, ref_lz = forward_backward(sc, [37] * 3)
        assert np.abs(ograd - ref).max() <= 1e-6 and np.abs(olz - ref_lz).max() <= 1e-6 * np.abs(ref_lz).max(), nb
        assert np.abs(ref.sum(2) - 1).max() < 1e-12


# ---------------------------------------------------------------------------------------------------------------------
# GPU: logZ and the posterior
# ---------------------------------------------------------------------------------------------------------------------
def _witness_columns(N):
    cols = []
    for lo in range(0, N, 64):
        cols += [lo, min(lo + 63, N - 1)]
    return sorted(set(cols))


def _scores(T, N, nb, kind, seed):
    """uniform on +-5 ("uniform"), or a trained network's confident scores, one alignment per read ("confident"): of 65
    reads, repeated along the batch (confident_scores walks every read's blocks in Python; with a period of 65 no two
    column groups hold the same read in the same lane)."""
    if kind == "uniform":
        return synth.scores(T, N, _nstate(nb), seed)
    n = min(N, 65)
    inp = synth.crf_case(T, n, seed, nbase=nb, seqlens=np.clip(synth.speedtest_seqlens(T, n), 1, T))
    sc = synth.confident_scores(inp, seed + 1, nbase=nb)["scores"]
    return np.ascontiguousarray(sc[:, np.arange(N) % n])


@functools.lru_cache(maxsize=2)
def _case(T, N, nb, kind):
    """The scores of a case, and on the witness columns the float64 posteriors and logZ with the fp32 oracle's beside
    them (computed once)."""
    import oracle
    sc = _scores(T, N, nb, kind, 2600 + 10 * T + N + nb)
    cols = _witness_columns(N)
    sub = np.ascontiguousarray(sc[:, cols])
    ref, ref_lz = forward_backward(sub, [T] * len(cols))
    olz, ograd = oracle.flipflop_logz_grad(sub)
    return sc, cols, ref, ref_lz, olz.astype(np.float64), ograd.astype(np.float64)


def _kind(k, nb):
    return ("uniform", "confident")[(k + nb) % 2]          # half and half, over the shapes and over the alphabet sizes


def _check_logz(oracle_mod, dev, T, N, nb, kind, want_plan):
    sc, cols, ref, ref_lz, olz, ograd = _case(T, N, nb, kind)
    plan = _lab_logz_plan(T, N, nb)                         # (under a lab switch: what that switch makes of the shape)
    assert plan == want_plan, (plan, want_plan)
    r = parity.compare_logz(oracle_mod, sc, dev)
    scale, lz_scale = np.abs(ref).max(), np.abs(ref_lz).max()
    e_hip, e_ora = np.abs(r["grad"][:, cols] - ref).max() / scale, np.abs(ograd - ref).max() / scale
    z_hip, z_ora = np.abs(r["logz"][cols] - ref_lz).max() / lz_scale, np.abs(olz - ref_lz).max() / lz_scale
    print("logz NB %d T %d N %d %s [%s]: oracle logZ rel %.3g posterior abs %.3g rows %.3g; float64 on %d columns: "
          "posterior %.3g (oracle %.3g), logZ %.3g (oracle %.3g)"
          % (nb, T, N, kind, _form(plan), r["logz_rel"], r["grad_abs"], r["rowsum_dev"], len(cols), e_hip, e_ora, z_hip, z_ora))
    assert r["finite"]
    assert r["logz_rel"] < LOSS_RTOL, r["logz_rel"]
    assert r["grad_abs"] < GRAD_ATOL, r["grad_abs"]
    assert r["rowsum_dev"] < 1e-5, r["rowsum_dev"]
    assert r["nograd_same"] == 0.0
    assert e_hip <= 2 * e_ora + 2e-6, (e_hip, e_ora)
    assert z_hip <= 2 * z_ora + 2e-6, (z_hip, z_ora)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NBASES)
@pytest.mark.parametrize("shape", list(LOGZ_SHAPES), ids=lambda s: "%dx%d" % s)
def test_logz_every_form_at_every_alphabet_size(oracle_mod, gpu_device, shape, nb):
    (T, N), k = shape, list(LOGZ_SHAPES).index(shape)
    assert not _lib.is_lab()                                # the release library, no switch
    plan = LOGZ_SHAPES[shape] + ((nb, LOGZ_SHAPES[shape][0]) in TAIL,)
    _check_logz(oracle_mod, gpu_device, T, N, nb, _kind(k, nb), plan)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NBASES)
def test_logz_smallest_shapes_at_every_alphabet_size(oracle_mod, gpu_device, nb):
    """A single row, one row less, exactly and one more than an 8-row chunk and than two; one read, a full column
    group, one read more."""
    assert not _lib.is_lab()
    for k, (T, N) in enumerate(SMALL_SHAPES):
        r = _check_logz(oracle_mod, gpu_device, T, N, nb, _kind(k, nb), (8, COOP, 8, (nb, 8) in TAIL))
        trans = decode.flipflop_make_trans(torch.from_numpy(_case(T, N, nb, _kind(k, nb))[0]).to(gpu_device))
        assert np.array_equal(trans.cpu().numpy(), r["grad"]), (T, N)       # the same launch behind the other entry point


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NBASES)
def test_make_trans_every_form_is_the_posterior(gpu_device, nb):
    """decode.flipflop_make_trans is the posterior launch of layers.flipflop_logpartition: the same bits, at the tail
    forms' shapes of both chunk sizes."""
    assert not _lib.is_lab()
    for T, N in ((50, 5), (883, 385)):
        sc = synth.scores(T, N, _nstate(nb), 77 + nb)
        _, grad = parity.run_logz(sc, gpu_device)
        trans = decode.flipflop_make_trans(torch.from_numpy(sc).to(gpu_device))
        assert not trans.requires_grad and np.array_equal(trans.cpu().numpy(), grad), (T, N, nb)


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NBASES)
def test_logz_streaming_transfer_at_every_alphabet_size(oracle_mod, gpu_device, nb, labenv):
    """logz_transfer_kernel<NB, 16, 0, true>: by shape alone it needs a 300 MB tensor; TK_K1_NT = 1 launches it here."""
    T, N = STREAM_SHAPE
    kind = _kind(list(LOGZ_SHAPES).index(STREAM_SHAPE), nb)
    plain = _lab_logz_plan(T, N, nb)
    labenv.setenv("TK_K1_NT", "1")
    assert plain == (16, PLAIN, 8, (nb, 16) in TAIL)
    r = _check_logz(oracle_mod, gpu_device, T, N, nb, kind, (16, STREAM, 8, (nb, 16) in TAIL))
    labenv.setenv("TK_K1_NT", "0")                          # ... and moves the same arithmetic: the plain form's bits
    lz0, g0 = parity.run_logz(_case(T, N, nb, kind)[0], gpu_device)
    assert np.array_equal(r["logz"], lz0) and np.array_equal(r["grad"], g0)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: the fused loss at the small alphabets (the accumulating store of the posterior kernel)
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nb", [2, 3])
def test_fused_loss_small_alphabets_at_sixteen_row_chunks(oracle_mod, gpu_device, nb):
    """ctc.flipflop_loss is the only route to logz_posterior_kernel<NB, 16, true> (NB 2: with the chains in the tail):
    the oracle's crf_flipflop_loss + logZ / T and its gradient, under the bounds of test_fused_loss_small_against_oracle.
    Ragged sequence lengths; an empty read only last (tests/helpers/fuzz_shapes.py)."""
    from taiyaki_amd import ctc
    T, N = FUSED_SHAPE
    plan = _lab_logz_plan(T, N, nb)
    assert plan == (16, COOP, 8, (nb, 16) in TAIL) and not _lib.is_lab()
    rng = np.random.RandomState(500 + nb)
    seqlens = np.clip(rng.randint(1, T // 2 + 1, size=N), 1, T).astype(np.int32)
    seqlens[:3] = (1, T // 2, 2)
    seqlens[-1] = 0
    inp = synth.crf_case(T, N, 510 + nb, nbase=nb, seqlens=seqlens)
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    lv = ctc.flipflop_loss(x, torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"]), 1.0)
    lv.sum().backward()
    oloss, ograd = oracle_mod.crf_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], 1.0)
    olz, olgrad = oracle_mod.flipflop_logz_grad(inp["scores"])
    want, got = (oloss + olz / T).astype(np.float64), lv.detach().cpu().numpy().astype(np.float64)
    gwant, ggot = ograd + olgrad / T, x.grad.cpu().numpy()
    print("fused loss NB %d T %d N %d [%s, accumulating store]: loss rel %.3g, gradient abs %.3g"
          % (nb, T, N, _form(plan), np.max(np.abs(got - want) / np.abs(want)), np.abs(ggot - gwant).max()))
    np.testing.assert_allclose(got, want, rtol=1e-5, atol=2e-6)
    np.testing.assert_allclose(ggot, gwant, atol=2e-5)


# ---------------------------------------------------------------------------------------------------------------------
# GPU: Viterbi
# ---------------------------------------------------------------------------------------------------------------------
def _viterbi_scores(T, N, nb, quantised, seed):
    sc = np.random.default_rng(seed).standard_normal((T, N, _nstate(nb)), dtype=np.float32) * np.float32(2)
    return (np.round(sc * 2) / 2).astype(np.float32) if quantised else sc           # a grid of 0.5: ties in nearly every step


def _check_viterbi(oracle_mod, dev, N, nb, waves, what):
    assert _lab_viterbi_plan(N) == waves, (N, waves)
    for T in VIT_STEPS[N]:
        for quantised in (True, False):
            sc = _viterbi_scores(T, N, nb, quantised, 1000 * T + 10 * N + 2 * nb + quantised)
            r = parity.compare_viterbi(oracle_mod, sc, dev)
            assert r["path_mismatch"] == 0 and r["tb_mismatch"] == 0 and r["fwd_bit_mismatch"] == 0, (T, N, nb, quantised)
            path_only = decode.flipflop_viterbi_path(torch.from_numpy(sc).to(dev)).cpu().numpy()
            assert np.array_equal(path_only, r["path"]), (T, N, nb, quantised)
    print("viterbi NB %d N %d [%s, %d waves per read; %s]: T %s, quantised and continuous: 0 mismatches in fwd bits, "
          "traceback and path" % (nb, N, what, waves, " and ".join(VIT_OUTPUTS), VIT_STEPS[N]))


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NBASES)
@pytest.mark.parametrize("N", list(VIT_BATCHES))
def test_viterbi_every_form_at_every_alphabet_size(oracle_mod, gpu_device, N, nb):
    assert not _lib.is_lab()
    _check_viterbi(oracle_mod, gpu_device, N, nb, VIT_BATCHES[N], "release rule")


@pytest.mark.gpu
@pytest.mark.parametrize("nb", NBASES)
@pytest.mark.parametrize("switch,waves", [("TK_VIT_V1", 1), ("TK_VIT_SPLIT", 3)])
def test_viterbi_every_step_count_meets_every_form(oracle_mod, gpu_device, switch, waves, nb, labenv):
    """The two large batches run five step counts; N = 11 through the one-wave and three-wave kernels runs all nine."""
    labenv.setenv(switch, "1")
    _check_viterbi(oracle_mod, gpu_device, 11, nb, waves, switch + "=1")


# ---------------------------------------------------------------------------------------------------------------------
# GPU: error probabilities at the C ABI
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("nb", NBASES)
def test_errprobs_inside_guards_against_float64(gpu_device, nb):
    """The block covers 8 time rows, two per wave, with a clamped odd last row; its columns are 64 reads with a clamped
    tail.  trans: positive random rows (every second case: one dominant entry per row); path: random states."""
    L, S, worst = _lib.lib(), _nstate(nb), 0.0
    bound = (S + 2 * nb + 4) * 2.0 ** -24
    into = [list(range(2 * nb * b, 2 * nb * (b + 1))) + [2 * nb * nb + b, 2 * nb * nb + nb + b] for b in range(nb)]
    for k, (N, T) in enumerate((N, T) for N in ERR_BATCHES for T in ERR_STEPS):
        rng = np.random.RandomState(100 * nb + k)
        trans = rng.uniform(0.01, 1.0, size=(T, N, S)).astype(np.float32)
        if k % 2:
            np.put_along_axis(trans, rng.randint(0, S, size=(T, N, 1)), np.float32(50.0), axis=2)
        path = rng.randint(0, 2 * nb, size=(T + 1, N)).astype(np.int64)
        flat, out = rows._guarded((T + 1, N), gpu_device, 0)
        tr, pth = torch.from_numpy(trans).to(gpu_device), torch.from_numpy(path).to(gpu_device)
        rc = L.tk_flipflop_errprobs_dev(_lib.ptr(tr), _lib.ptr(pth), T, N, nb, _lib.ptr(out), _lib.stream_ptr())
        _lib.check(rc, "tk_flipflop_errprobs_dev")
        torch.cuda.synchronize()
        assert rows._guards_intact(flat, 0, out.numel()), (N, T, "a store outside the tensor")
        got = out.cpu().numpy()
        assert not (got == rows.SENTINEL).any(), (N, T, "elements not stored")
        assert (got[0] == -1.0).all(), (N, T)
        base = np.stack([trans[:, :, idx].astype(np.float64).sum(axis=2) for idx in into], axis=2)
        p = np.take_along_axis(base, (path[1:] % nb)[:, :, None], axis=2)[:, :, 0]
        want = 1.0 - p / (base.sum(axis=2) + 1e-10)
        err = float(np.abs(got[1:] - want).max())
        assert err <= bound, (N, T, err, bound)
        worst = max(worst, err)
    print("errprobs NB %d [errprobs_kernel<%d>; N %s x T %s]: largest error %.3g, bound (S + 2NB + 4) 2^-24 = %.3g"
          % (nb, nb, ERR_BATCHES, ERR_STEPS, worst, bound))
