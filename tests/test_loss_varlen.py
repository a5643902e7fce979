"""The flip-flop loss with a time length per column (include/taiyaki_amd_loss_varlen.h; `lengths=` of the ctc operators) on the
GPU.  Every expected value comes from the oracle ONE COLUMN AT A TIME, on scores[:T_n, n:n+1] with that read's labels:
oracle.crf_flipflop_loss / cat_mod_flipflop_loss (the reference's float32 arithmetic), oracle.crf_flipflop_loss_f64 (the
float64 witness) and oracle.flipflop_logz_grad.  Bounds: tests/parity.py's crf_loss_ok and crf_grad_ok on the posterior scale
(gradient x T_n), for the fused forms those of tests/test_gpu_parity.py's fused tests (loss rtol 1e-5 / atol 2e-6, gradient
2e-5 x the read's weight) -- no bound of this file's own.  A case is named by what tk_crf_varlen_plan reports for it.

Before a linear-path case is judged, the EXISTING call on each column alone must report 0 reads retried and 0 redone in the
log domain (labels of at most 0.5 T_n on scores in the network's 5 tanh range); the call with lengths must then report 0 and 0
too, so that the tail launch cannot hide a wrong sweep.  The tail-launch cases compare the counts instead."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, ctc, layers, synth
from tests import parity

pytestmark = pytest.mark.gpu

MODS = (1, 1, 0, 0)
NBLK = 61
PLAN_FIELDS = ("log_domain", "log_R", "log_W", "log_CK", "R", "W", "BK", "bias2", "slope", "rows", "wcap", "retry_BK", "retry_bias2",
               "retry_slope", "retry_R", "retry_W", "side_by_side", "tail_log_R", "slots", "tail_R")
# (form, sharpening factor) -> the block length the launch takes at nblk 61
FORMS = {("plain", 1.0): 12, ("plain", 1.5): 8, ("plain", 2.5): 4, ("catmod", 1.0): 8, ("catmod", 2.5): 4}


def plan(ntrans, nblk, nbatch, max_seqlen, bulk, catmod, want_grad, sharp):
    """tk_crf_varlen_plan for a call whose workspace is the library's own query: a dict over PLAN_FIELDS."""
    wsb = _lib.lib().tk_crf_flipflop_workspace_bytes_sharp(ntrans, nblk, nbatch, max_seqlen, int(want_grad), float(sharp))
    out = (ctypes.c_size_t * 20)()
    assert _lib.loss_varlen_lib().tk_crf_varlen_plan(ntrans, nblk, nbatch, max_seqlen, bulk, int(catmod), int(want_grad),
                                                     float(sharp), wsb, out)
    return dict(zip(PLAN_FIELDS, (int(v) for v in out)))


def lengths_for(bk, second):
    """0, 1, BK - 1, BK, BK + 1, a multiple of BK, nblk - 1 and nblk over two batches of seven columns."""
    if not second:
        return [0, 1, bk - 1, bk, bk + 1, NBLK - 1, NBLK]
    return [(NBLK // bk) * bk, NBLK, 1, bk + 1, 0, 2 * bk, NBLK - 1]


def ragged_case(nblk, lengths, seed, catmod, seqlens=None):
    """Scores in the 5 tanh range and labels of 1 base up to 0.5 T_n (a column without rows keeps one label)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    if seqlens is None:
        seqlens = np.maximum(1, lengths // 2)
        seqlens[len(lengths) // 2] = 1
    inp = synth.crf_case(nblk, len(lengths), seed, nmods_per_base=MODS if catmod else None, seqlens=seqlens)
    if catmod:
        synth.normalise_mod_columns(inp)        # (what the producer layer emits: log-probabilities in the category columns)
    inp["lengths"] = lengths
    return inp


def column(inp, n):
    """Column n alone at its own length: the inputs of a fixed-length call."""
    off = np.concatenate([[0], np.cumsum(inp["seqlens"])])
    T_n = int(inp["lengths"][n])
    out = dict(scores=np.ascontiguousarray(inp["scores"][:T_n, n:n + 1]), seqs=inp["seqs"][off[n]:off[n + 1]],
               seqlens=inp["seqlens"][n:n + 1])
    if "mod_cats" in inp:
        out.update(mod_cats=inp["mod_cats"][off[n]:off[n + 1]], can_mods_offsets=inp["can_mods_offsets"],
                   mod_cat_weights=inp["mod_cat_weights"])
    return out


def expected(oracle, inp, sharp, fused=False):
    """Per column from the oracle: loss (N), gradient of the float32 oracle and of the float64 witness (T, N, S), zeros at and
    beyond T_n and for a column without rows.  fused: + logZ_n / T_n on the canonical columns."""
    T, N, S = inp["scores"].shape
    loss, g32, g64 = np.zeros(N), np.zeros((T, N, S)), np.zeros((T, N, S))
    for n in range(N):
        T_n = int(inp["lengths"][n])
        if T_n == 0 or inp["seqlens"][n] == 0:
            continue
        col = column(inp, n)
        ol, og = parity.oracle_crf(oracle, col, sharp)
        _, wg = parity.oracle_crf_f64(oracle, col, sharp)
        loss[n], g32[:T_n, n], g64[:T_n, n] = ol[0], og[:, 0], wg[:, 0]
        if fused:
            lz, lg = oracle.flipflop_logz_grad(np.ascontiguousarray(col["scores"][:, :, :40]))
            loss[n] += lz[0] / T_n
            g32[:T_n, n, :40] += lg[:, 0] / T_n
            g64[:T_n, n, :40] += lg[:, 0] / T_n
    return loss, g32, g64


def run(inp, sharp, dev, want_grad=True, lengths="own", fused=False, weights=None, scores=None, bulk_unknown=False):
    """The operator with `lengths` (own: the case's; None: without the keyword) -> loss (N), gradient or None, retried, redone.
    bulk_unknown: the lengths carry their maximum and no bulk (ctc.set_max_seqlen): the launch takes the fast configuration."""
    x = torch.from_numpy(inp["scores"] if scores is None else scores).to(dev).requires_grad_(want_grad)
    seqs, seqlens = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"])
    if bulk_unknown:
        seqlens = ctc.set_max_seqlen(seqlens, int(inp["seqlens"].max()))
    kw = {} if lengths is None else dict(lengths=inp["lengths"] if isinstance(lengths, str) else lengths)
    mods = ()
    if "mod_cats" in inp:
        mods = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"])
    if fused:
        w = None if weights is None else torch.from_numpy(weights).to(dev)
        total, loss = ctc.flipflop_mean_loss(x, seqs, seqlens, sharp, w, *(mods or (None, None, None)), **kw)
    elif mods:
        loss = ctc.cat_mod_flipflop_loss(x, seqs, seqlens, *mods, sharp, **kw)
        total = loss.sum()
    else:
        loss = ctc.crf_flipflop_loss(x, seqs, seqlens, sharp, **kw)
        total = loss.sum()
    counts = (ctc.last_retry_count(), ctc.last_gate_count())
    grad = None
    if want_grad:
        total.backward()
        grad = x.grad.detach().cpu().numpy()
    return loss.detach().cpu().numpy(), grad, counts[0], counts[1]


@functools.lru_cache(maxsize=None)
def alone_counts(form, sharp, second, nblk=NBLK):
    """The existing call on every column of the case alone: (retried, redone) summed -- run once per case."""
    dev = torch.device("cuda:0")
    inp = ragged_case(nblk, lengths_for(FORMS[form, sharp], second), 40 + int(10 * sharp), form == "catmod")
    return _alone_counts(inp, sharp, dev)


def _alone_counts(inp, sharp, dev, **kw):
    retried = redone = 0
    for n in range(len(inp["lengths"])):
        if inp["lengths"][n] == 0:
            continue
        _, _, a, b = run(column(dict(inp, lengths=inp["lengths"]), n), sharp, dev, lengths=None, **kw)
        retried, redone = retried + a, redone + b
    return retried, redone


def judge_crf(inp, sharp, loss, grad, want, what):
    """parity.crf_loss_ok / crf_grad_ok on the posterior scale: gradient x T_n, modification columns over their weight."""
    oloss, g32, g64 = want
    r = dict(loss=loss, oloss=oloss)
    print("%s: loss rel %.3g" % (what, parity.rel_err(loss[oloss != 0], oloss[oloss != 0])))
    assert np.isfinite(loss).all() and parity.crf_loss_ok(r), (what, loss, oloss)
    if grad is None:
        return
    ps = parity.posterior_scale(inp)[None, None, :] * inp["lengths"][None, :, None]
    r.update(grad_f64_scaled=parity.abs_err(grad * ps, g64 * ps), ref_noise_scaled=parity.abs_err(g32 * ps, g64 * ps),
             grad_scaled_abs=parity.abs_err(grad * ps, g32 * ps))
    print("%s: gradient x T_n vs float64 %.3g, vs the oracle %.3g, the oracle's own distance %.3g" % (
        what, r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"]))
    assert np.isfinite(grad).all() and parity.crf_grad_ok(r), (what, r["grad_f64_scaled"], r["grad_scaled_abs"], r["ref_noise_scaled"])


def assert_padding_zero(inp, grad, what):
    beyond = np.arange(grad.shape[0])[:, None] >= inp["lengths"][None, :]
    assert not grad[beyond].any(), (what, "gradient rows at or beyond T_n are not exactly 0")
    dead = (inp["lengths"] == 0) | (inp["seqlens"] == 0)
    assert not grad[:, dead].any(), (what, "a column without rows or labels has a gradient")


# ---------------------------------------------------------------------------------------------------------------------
# 1. ragged batches against the oracle
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("second", [False, True])
@pytest.mark.parametrize("form,sharp", sorted(FORMS))
def test_ragged_batch_against_the_oracle(oracle_mod, gpu_device, form, sharp, second):
    bk, catmod = FORMS[form, sharp], form == "catmod"
    inp = ragged_case(NBLK, lengths_for(bk, second), 40 + int(10 * sharp), catmod)
    S, N = inp["scores"].shape[2], len(inp["lengths"])
    for g in (0, 1):
        p = plan(S, NBLK, N, int(inp["seqlens"].max()), ctc.bulk_of(inp["seqlens"]), catmod, g, sharp)
        assert p["log_domain"] == 0 and p["BK"] == bk, p
    what = "%s x%.1f BK %d lengths %s" % (form, sharp, bk, inp["lengths"].tolist())
    assert alone_counts(form, sharp, second) == (0, 0), (what, "precondition: the existing call on a column alone retried or redid a read")
    want = expected(oracle_mod, inp, sharp)
    # cost only, cost and gradient
    loss0, _, retried, redone = run(inp, sharp, gpu_device, want_grad=False)
    assert (retried, redone) == (0, 0), what
    judge_crf(inp, sharp, loss0, None, want, what + " cost only")
    loss, grad, retried, redone = run(inp, sharp, gpu_device)
    assert (retried, redone) == (0, 0), what
    judge_crf(inp, sharp, loss, grad, want, what + " gradient")
    assert_padding_zero(inp, grad, what)
    assert not loss[(inp["lengths"] == 0)].any() and not loss0[(inp["lengths"] == 0)].any()
    # fused, and fused with a weight per read: the bounds of test_gpu_parity's fused tests
    wloss, wg32, _ = expected(oracle_mod, inp, sharp, fused=True)
    rs = np.random.RandomState(5)
    for weights in (None, (rs.uniform(0.2, 1.0, size=N) / N).astype(np.float32)):
        lv, fg, retried, redone = run(inp, sharp, gpu_device, fused=True, weights=weights)
        assert (retried, redone) == (0, 0), what
        w = np.full(N, 1.0 / N) if weights is None else weights.astype(np.float64)
        np.testing.assert_allclose(lv, wloss, rtol=1e-5, atol=2e-6, err_msg=what + " fused")
        err = np.abs(fg - wg32 * w[None, :, None]).max(axis=(0, 2)) / w
        print("%s fused%s: gradient error over the weight, per column %s" % (what, "" if weights is None else " weighted", err))
        assert np.isfinite(fg).all() and (err <= 2e-5).all(), (what, err)
        assert_padding_zero(inp, fg, what + " fused")
        assert not lv[(inp["lengths"] == 0)].any()


# ---------------------------------------------------------------------------------------------------------------------
# 2. padding is written and inert
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form,sharp", sorted(FORMS))
def test_padding_is_written_and_inert(gpu_device, form, sharp, monkeypatch):
    """NaN in the scores beyond T_n changes no bit of any output and sets no status bit (strict mode raises on one); the
    gradient rows there come back exactly 0 although the operator's gradient tensor is filled with NaN before the call."""
    real_empty_like = torch.empty_like
    monkeypatch.setattr(torch, "empty_like", lambda t, **kw: real_empty_like(t, **kw).fill_(float("nan")) if t.is_floating_point()
                        else real_empty_like(t, **kw))
    bk, catmod = FORMS[form, sharp], form == "catmod"
    inp = ragged_case(NBLK, lengths_for(bk, True), 40 + int(10 * sharp), catmod)
    poisoned = inp["scores"].copy()
    poisoned[np.arange(NBLK)[:, None] >= inp["lengths"][None, :]] = np.nan
    assert np.isnan(poisoned).any()
    for fused in (False, True):
        clean = run(inp, sharp, gpu_device, fused=fused)
        dirty = run(inp, sharp, gpu_device, fused=fused, scores=poisoned)
        assert clean[2:] == dirty[2:] == (0, 0)
        assert np.array_equal(clean[0].view(np.uint32), dirty[0].view(np.uint32)), (form, sharp, fused, "loss")
        assert np.array_equal(clean[1].view(np.uint32), dirty[1].view(np.uint32)), (form, sharp, fused, "gradient")
        assert_padding_zero(inp, dirty[1], (form, sharp, fused))
        cost_clean = run(inp, sharp, gpu_device, want_grad=False)[0]
        cost_dirty = run(inp, sharp, gpu_device, want_grad=False, scores=poisoned)[0]
        assert np.array_equal(cost_clean.view(np.uint32), cost_dirty.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------------------
# 3. lengths = NULL, [nblk] * N and a uniform T' < nblk: the existing call bit for bit
# ---------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return None if a is None else a.view(np.uint32)


@pytest.mark.parametrize("want_grad", [False, True])
@pytest.mark.parametrize("form,sharp", sorted(FORMS))
def test_full_and_uniform_lengths_are_the_existing_call_bit_for_bit(gpu_device, form, sharp, want_grad):
    catmod = form == "catmod"
    N, Tp = 7, 37
    seqlens = np.array([18, 1, 7, 12, 3, 16, 9])          # (at most 0.5 T': the same labels serve both shapes)
    inp = ragged_case(NBLK, [NBLK] * N, 70 + int(10 * sharp), catmod, seqlens=seqlens)
    S = inp["scores"].shape[2]
    want = run(inp, sharp, gpu_device, want_grad=want_grad, lengths=None)
    assert want[2:] == (0, 0)
    # the C entry itself with lengths == NULL and with [nblk] * N (status word 0: no flag, nothing retried or redone), and
    # the operator with [nblk] * N
    null = crf_abi(inp, sharp, gpu_device, want_grad, None)
    full_abi = crf_abi(inp, sharp, gpu_device, want_grad, [NBLK] * N)
    assert null[2] == 0 and full_abi[2] == 0, (null[2], full_abi[2])
    full = run(inp, sharp, gpu_device, want_grad=want_grad, lengths=[NBLK] * N)
    assert full[2:] == (0, 0)
    for got, name in ((null, "lengths = NULL"), (full_abi, "lengths = [nblk] * N, C entry"), (full, "lengths = [nblk] * N")):
        assert np.array_equal(_bits(got[0]), _bits(want[0])), (form, sharp, name, "loss")
        assert want[1] is None or np.array_equal(_bits(got[1]), _bits(want[1])), (form, sharp, name, "gradient")
    # a uniform T' < nblk against the existing call on a contiguous copy of scores[:T'], where the two plans are equal
    mx, bulk = int(seqlens.max()), ctc.bulk_of(seqlens)
    p_full, p_short = (plan(S, t, N, mx, bulk, catmod, want_grad, sharp) for t in (NBLK, Tp))
    assert p_full == p_short and p_full["BK"] == FORMS[form, sharp], (p_full, p_short)
    short = dict(inp, scores=np.ascontiguousarray(inp["scores"][:Tp]), lengths=np.full(N, Tp))
    want = run(short, sharp, gpu_device, want_grad=want_grad, lengths=None)
    got = run(inp, sharp, gpu_device, want_grad=want_grad, lengths=[Tp] * N)
    assert want[2:] == got[2:] == (0, 0)
    assert np.array_equal(_bits(got[0]), _bits(want[0])), (form, sharp, "uniform T'", "loss")
    if want_grad:
        assert np.array_equal(_bits(got[1][:Tp]), _bits(want[1])) and not got[1][Tp:].any(), (form, sharp, "uniform T'")


def crf_abi(inp, sharp, dev, want_grad, lengths):
    """tk_crf_flipflop_varlen_labels_dev itself, with the arguments ctc._run gives it, on outputs filled with NaN; `lengths`
    None: the NULL pointer.  -> cost (N), gradient or None, the status word."""
    V, L = _lib.loss_varlen_lib(), _lib.lib()
    lp = torch.from_numpy(inp["scores"]).to(dev)
    nblk, nbatch, ntrans = lp.shape
    catmod = "mod_cats" in inp
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    mods = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"]) if catmod else (None, None, None)
    seqlen_d, seqoff, stay, move, mod, fact, keep, labels = ctc._indices(
        torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"]), 4, dev, *mods, status=status, defer=True)
    maxlen = int(inp["seqlens"].max())
    cost = torch.full((nbatch,), float("nan"), device=dev)
    grad = torch.full_like(lp, float("nan")) if want_grad else None
    wsb = L.tk_crf_flipflop_workspace_bytes_sharp(ntrans, nblk, nbatch, maxlen, int(want_grad), float(sharp))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    lens = None if lengths is None else torch.tensor(lengths, dtype=torch.int32, device=dev)
    rc = V.tk_crf_flipflop_varlen_labels_dev(
        _lib.ptr(lp), ntrans, nblk, nbatch, ctypes.byref(labels), _lib.ptr(seqlen_d), _lib.ptr(seqoff), _lib.ptr(stay),
        _lib.ptr(move), _lib.ptr(mod), _lib.ptr(fact), maxlen, 40, float(sharp), 1.0 if catmod else float(sharp), 1.0 / sharp,
        _lib.ptr(cost), _lib.ptr(grad), _lib.ptr(ws), wsb, _lib.ptr(status), _lib.stream_ptr(), _lib.ptr(lens))
    assert rc == 0, rc
    torch.cuda.synchronize()
    del keep
    return cost.cpu().numpy(), None if grad is None else grad.cpu().numpy(), int(status.item()) & 0xffffffff


# ---------------------------------------------------------------------------------------------------------------------
# 4. more than one chunk wave and more than one cell per lane
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nblk,L0,field,value", [(2100, 600, "W", None), (2100, 1100, "R", 2), (2100, 2080, "R", 4),
                                                 (4200, 2080, "R", 4)])
def test_long_reads_against_float64(oracle_mod, gpu_device, nblk, L0, field, value):
    """nblk 2100: a read of L0 bases in a column of 2100 rows beside 500 bases in a column of 1300 rows -- the smallest
    shapes with several chunk waves (600), two (1100) and four (2080) cells per lane.  The 2080-base read's band is 22 cells
    wide there: the existing call on that column alone hands it to the tail launch, the counts must equal that call's, and
    what is judged may be the tail launch's rows.  So the same read once more in a column of 4200 rows beside one of 2600
    (0.5 T_n): four cells per lane with nothing retried, the batch sweep's own output.  Gradient call and cost-only call
    each against the counts of per-column calls of their own form."""
    sharp = 1.0
    inp = ragged_case(nblk, [nblk, nblk * 13 // 21], 90, False, seqlens=np.array([L0, 500]))
    want = expected(oracle_mod, inp, sharp)
    for want_grad in (True, False):
        p = plan(40, nblk, 2, L0, ctc.bulk_of(inp["seqlens"]), False, want_grad, sharp)
        assert p["log_domain"] == 0 and (p["W"] > 1 if value is None else p[field] == value), p
        counts = _alone_counts(inp, sharp, gpu_device, want_grad=want_grad)
        assert (nblk, L0) == (2100, 2080) or counts == (0, 0), (want_grad, counts)
        loss, grad, retried, redone = run(inp, sharp, gpu_device, want_grad=want_grad)
        print("nblk %d L0 %d %s: retried %d, redone %d; the columns alone %s" % (
            nblk, L0, "gradient" if want_grad else "cost only", retried, redone, counts))
        assert (retried, redone) == counts, (want_grad, (retried, redone), counts)
        judge_crf(inp, sharp, loss, grad, want, "nblk %d L0 %d plan %s" % (nblk, L0, {k: p[k] for k in ("R", "W", "BK", "rows", "wcap")}))
        if want_grad:
            assert_padding_zero(inp, grad, L0)


# ---------------------------------------------------------------------------------------------------------------------
# 5. the tail launch with lengths
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["plain", "catmod"])
def test_tail_launch_with_lengths(oracle_mod, gpu_device, form):
    """One read of 0.95 T_n bases among ordinary ones, every launch at the fast configuration (the batch's bulk is ordinary;
    the calls on single columns are told no bulk): the existing call on that column alone retries it, and the call with
    lengths retries (and redoes) as many as the per-column calls together."""
    nblk, sharp, catmod = 860, 1.0, form == "catmod"
    lengths = np.array([860, 800, 500, 300, 0])
    seqlens = np.array([300, 760, 200, 100, 5])           # column 1: 0.95 T_n
    inp = ragged_case(nblk, lengths, 33, catmod, seqlens=seqlens)
    # (no bulk: the fast configuration, 12-step blocks for both forms -- cat-mod from 705 bases on -- and a retry at 4)
    for g in (0, 1):
        p = plan(inp["scores"].shape[2], nblk, len(lengths), int(seqlens.max()), 0, catmod, g, sharp)
        assert (p["log_domain"], p["BK"], p["retry_BK"]) == (0, 12, 4), p
    _, _, r1, g1 = run(column(inp, 1), sharp, gpu_device, lengths=None, bulk_unknown=True)
    assert r1 >= 1, "the existing call keeps this read on the batch launch: not a tail-launch case"
    want = expected(oracle_mod, inp, sharp)
    for want_grad in (False, True):
        counts = _alone_counts(inp, sharp, gpu_device, bulk_unknown=True, want_grad=want_grad)
        loss, grad, retried, redone = run(inp, sharp, gpu_device, want_grad=want_grad, bulk_unknown=True)
        assert (retried, redone) == counts, (form, want_grad, (retried, redone), counts)
        judge_crf(inp, sharp, loss, grad, want, "%s tail launch (retried %d, redone %d)" % (form, retried, redone))
        if want_grad:
            assert_padding_zero(inp, grad, form)


# ---------------------------------------------------------------------------------------------------------------------
# 6. the Python layer
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
def test_mean_loss_with_lengths_is_the_sum_of_the_columns(gpu_device, weighted):
    """flipflop_mean_loss(..., lengths=) against the existing operator on every column alone, weights included: loss and
    gradient, under the bounds of test_mean_loss_operator_hands_over_the_final_gradient (1e-5 / 2e-6; 2e-5 x the weight)."""
    nblk = 90
    inp = ragged_case(nblk, [90, 0, 45, 13, 77, 1], 21, False)
    N = len(inp["lengths"])
    w = (np.linspace(0.5, 1.5, N) / N).astype(np.float32) if weighted else np.full(N, 1.0 / N, dtype=np.float32)
    x = torch.from_numpy(inp["scores"]).to(gpu_device).requires_grad_()
    loss, lv = ctc.flipflop_mean_loss(x, torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"]), 1.0,
                                      torch.from_numpy(w).to(gpu_device) if weighted else None, lengths=inp["lengths"])
    loss.backward()
    want_loss, want_grad = 0.0, np.zeros(inp["scores"].shape)
    for n in range(N):
        T_n = int(inp["lengths"][n])
        if T_n == 0:
            continue
        col = column(inp, n)
        xc = torch.from_numpy(col["scores"]).to(gpu_device).requires_grad_()
        lc = ctc.flipflop_loss(xc, torch.from_numpy(col["seqs"]), torch.from_numpy(col["seqlens"]), 1.0)
        (lc.sum() * float(w[n])).backward()
        want_loss += float(lc.detach().sum()) * float(w[n])
        want_grad[:T_n, n] = xc.grad[:, 0].cpu().numpy()
        assert abs(float(lv[n]) - float(lc[0])) <= 1e-5 * abs(float(lc[0])) + 2e-6, (n, float(lv[n]), float(lc[0]))
    assert abs(float(loss) - want_loss) <= 1e-5 * abs(want_loss) + 2e-6
    err = np.abs(x.grad.cpu().numpy() - want_grad).max(axis=(0, 2)) / w
    print("gradient error over the weight, per column:", err)
    assert (err <= 2e-5).all(), err
    assert_padding_zero(inp, x.grad.cpu().numpy(), "mean loss")


@pytest.mark.parametrize("fused", [True, False])
def test_calculate_loss_with_lengths(oracle_mod, gpu_device, fused, monkeypatch):
    """train.calculate_loss(..., lengths=) on mGru_flipflop(size=32): T 200, N 4, lengths 200 / 137 / 64 / 0, with
    train.FUSED_LOSS on and off.  The rule of tests/test_rnn_varlen_train.py's layer tests (_compare_with_columns_alone):
    against a float64 witness, err <= 2 err_alone + 2e-6, each error over the tensor's largest entry -- for the loss and every
    parameter gradient.  The witness: the network in double on the CPU, column by column, its backward driven by the
    float64 loss gradient of that column's outputs (oracle.crf_flipflop_loss_f64 + the float64 log-partition of
    tests/test_decode_varlen.py over T_n); alone: per-column calculate_loss runs on the device, summed."""
    import copy
    from taiyaki_amd import models, train
    from tests.test_decode_varlen import forward_backward
    monkeypatch.setattr(layers, "TRAIN_VARLEN", True)
    monkeypatch.setattr(train, "FUSED_LOSS", fused)
    T, lens, stride = 200, [200, 137, 64, 0], 5
    torch.manual_seed(4)
    net = synth.excite_network(models.mGru_flipflop(size=32, stride=stride))
    n64 = copy.deepcopy(net).double()
    net = net.to(gpu_device)
    xh = torch.randn(T, len(lens), 1, generator=torch.Generator().manual_seed(6))
    for n, ln in enumerate(lens):
        xh[ln:, n] = 0
    x = xh.to(gpu_device)
    out_lens = [-(-ln // stride) for ln in lens]
    seqlens = np.array([max(1, t // 2) for t in out_lens])
    seqs, _ = synth.sequences(seqlens.astype(np.int32), 8)
    off = np.concatenate([[0], np.cumsum(seqlens)])
    N = len(lens)

    def grads(module=None):
        module = net if module is None else module
        out = {k: p.grad.detach().double().cpu().clone() for k, p in module.named_parameters() if p.grad is not None}
        module.zero_grad(set_to_none=True)
        return out
    loss, lv = train.calculate_loss(net, x, torch.from_numpy(seqs), torch.from_numpy(seqlens), lengths=lens)
    loss.backward()
    got, got_loss = grads(), float(loss.detach())
    assert float(lv[3]) == 0.0
    alone, alone_loss, ref, ref_loss = {}, 0.0, {}, 0.0
    for n in range(N):
        if lens[n] == 0:
            continue
        col_seqs, col_len = seqs[off[n]:off[n + 1]], seqlens[n:n + 1]
        lc, _ = train.calculate_loss(net, x[:lens[n], n:n + 1].contiguous(), torch.from_numpy(col_seqs), torch.from_numpy(col_len))
        (lc / N).backward()
        alone_loss += float(lc.detach()) / N
        for k, v in grads().items():
            alone[k] = alone.get(k, 0) + v
        # the float64 witness of this column
        out = n64(xh[:lens[n], n:n + 1].double())
        sc = out.detach().numpy()
        assert sc.shape == (out_lens[n], 1, 40)
        wl, wg = oracle_mod.crf_flipflop_loss_f64(sc, col_seqs, col_len, 1.0)
        trans, lz = forward_backward(sc, [out_lens[n]])
        ref_loss += (float(wl[0]) + float(lz[0]) / out_lens[n]) / N
        out.backward(torch.from_numpy((wg + trans / out_lens[n]) / N))
        for k, v in grads(n64).items():
            ref[k] = ref.get(k, 0) + v
    assert set(got) == set(alone) == set(ref) and len(got) >= 10, (sorted(got), sorted(ref))
    e, e_alone = abs(got_loss - ref_loss) / abs(ref_loss), abs(alone_loss - ref_loss) / abs(ref_loss)
    print("loss %.7g, the columns alone %.7g, float64 %.9g: err %.3e, alone %.3e" % (got_loss, alone_loss, ref_loss, e, e_alone))
    assert e <= 2 * e_alone + 2e-6, (e, e_alone)
    for k, r in ref.items():
        scale = r.abs().max().item()
        assert scale > 0, k
        e, e_alone = (got[k] - r).abs().max().item() / scale, (alone[k] - r).abs().max().item() / scale
        print("%s: batched %.3e, columns alone %.3e, ratio %.3f" % (k, e, e_alone, e / (2 * e_alone + 2e-6)))
        assert e <= 2 * e_alone + 2e-6, (k, e, e_alone)
