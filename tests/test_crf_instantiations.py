"""Every instantiation of kernel A -- the flip-flop CRF loss and gradient (csrc/crf_band.hip, crf_band_posterior.inc,
crf_log.h, crf_kernels.hip) -- launched at least once and compared with the C oracle and the float64 witness.

The table (TABLE below, 85 entries):

  ("sweep", R, form, BK, ROWS, WCAP)   crf_band_sweep_kernel: cells per lane 1 / 2 / 4; form 0 the plain CRF, 1 cat-mod with
                                       per-column factors, 2 cat-mod with per-position factors ("general"); block length
                                       4 / 8 / 12 (no 12 for the general form); with a row-maker wave or without (8- and
                                       12-step blocks of forms 0 and 1 only); wave-count class 8 / 12 / 16 at four cells per
                                       lane and blocks of 8 or 12 steps, else 16                        23 + 23 + 8 = 54
  ("post", form, BK)                   crf_band_posterior_kernel                                         3 + 3 + 2 =  8
  ("tail", R, form)                    crf_band_tail_kernel: the retry at 4-step blocks, then crf_read<2 or 4, 16>      9
  ("log", R, W, cat-mod)               crf_kernel, the log-domain form on every read: (1,1) (2,1) (2,2) (2,4) (2,8)
                                       (2,16) (4,16)                                                              7 x 2 = 14

A case names the entry it runs, never only a shape: the launchers take their choices from small host functions
(crf_kernels.hip: crf_choose; crf_band.hip: crf_band_pick_R, crf_band_pick_block, crf_band_pick_retry, crf_band_retry_R,
crf_band_use_rows, crf_band_wave_class) that the lab build reports through tk_lab_crf_plan.  The CPU tests restate those
rules in Python (`plan_rule`), hold the restatement against the library on both sides of every threshold, assert that the
GPU case tables reach all 85 entries -- the entry of a case is the one the plan query reports for the call the operator
makes -- and mark which entries the release rule reaches with no lab switch (LAB_ONLY: the others).  `plan_rule` does not
restate the workspace layout's byte counts: the form follows the workspace only through TK_CRF_LATTICE_MB = 0 here.

GPU cases, all through the Python operators:
  (a) LOG_CASES   the log-domain kernel on every read (TK_CRF_MODE=ckpt), seven shapes x plain / cat-mod: per shape a batch
      whose longest read is one base into the shape's range and one at its capacity, the longest read being L = T + 1, with
      reads of 1, 64 and 65 bases beside it; and, for the shapes at which the checkpoint spacing CK changes, a batch with
      T = the first length of the range, so that T mod CK takes 0 (first batch), CK - 1 (second) and 1 (third) at each of
      CK = 16, 8, 4, 2.  Gradient call and cost-only call.
  (b) BAND_CASES  the linear path: every sweep and gradient-pass instantiation, R / BK / bias / feed through the lab
      switches, the general form through TK_CATMOD_GENERAL; reads that end one before, on and one after a chunk boundary
      (64 R) and one in the launch's top chunk wave, T no multiple of 4, 8 or 12.  The wave-count classes 12 and 16 of the
      small batches come from the max_seqlen hint alone; HEAVY_CASES reach each class's top wave with a read that long,
      once per form.  Every case asserts that NOTHING was retried or redone: a sweep that is wrong disagrees with its twin,
      and the fallback's answer would hide it.  The two feeds of a configuration must give the same bits.
  (c) TAIL_CASES  the tail launch, nine instantiations: ordinary reads with bands 2 - 12 cells wide (crf_read's, from T ~ 500
      on) and of 3 - 9 % of T (the retry's) among them, lengths without
      a bulk length, longest read <= 512, 513 - 1024, 1025 - 2048 (the retry at four cells per lane, sweeps side by side) and
      beyond 2048 (one sweep after the other); as shipped (retried >= 1), without the retry (TK_CRF_NO_RETRY=1: redone =
      disowned >= 1, by crf_read) and without the fallback on poisoned outputs (TK_CRF_NO_FALLBACK=1: what the retry keeps
      is finite and the shipped run's bits, and there is such a read); gradient call and cost-only call.

Criteria, the project's own: the loss by parity.crf_loss_ok against the C oracle (T <= 1100) or against the witness; the
gradient on the posterior scale within parity.GRAD_T_ATOL of the float64 WITNESS, with no allowance for the reference's
noise (the inputs are the plain CRF and cat-mod on synth.normalise_mod_columns scores); NOISE_ALLOWED lists the cases
that fall back to parity.crf_grad_ok, with their figures.  Every case prints one line that starts with "r27|";
profiles/r27_crf_instantiations.txt keeps one run.  After a launch that raised, this module launches nothing more (the
remaining tests fail at once).

What this file found when it was written: no instantiation computes a wrong number (linear path at most 2.2e-6 from float64,
crf_kernel 2.7e-5, reads redone by crf_read in the tail 2.5e-4).  Four sweep instantiations are reached by a lab switch only
(LAB_ONLY).  Cat-mod with per-column factors at four cells per lane and the release rule's 12-step blocks disowns every read of
a batch of synth.confident_scores and retries it (right answers, one read per workgroup): the heavy cat-mod cases run iid
scores for that reason, LABNOTES has the figures.  That the cases bite was tried on three scratch builds with one arithmetic
mutation each: crf_read at CK = 2 (17 cases here fail, and 20 earlier cat-mod tests), the tail's sequential branch (the three
tail-r4seq cases, no earlier test), the class-16 sweep at four cells per lane (eight cases, no earlier test)."""
import ctypes
import functools
import itertools
import os

import numpy as np
import pytest

from taiyaki_amd import _lib, synth
from tests import parity

PLAIN, COLW, GENERAL = 0, 1, 2
FORM_NAMES = ("plain", "cat-mod per column", "cat-mod general")
MODS = (1, 1, 0, 0)
WAVE, MAXW, KLIP, ROW_PITCH = 64, 16, 6, 48
LOG_SHAPES = [(1, 1), (2, 1), (2, 2), (2, 4), (2, 8), (2, 16), (4, 16)]


# ---------------------------------------------------------------------------------------------------------------------
# the table
# ---------------------------------------------------------------------------------------------------------------------
def _sweep_entries(form):
    out = []
    for R in (1, 2, 4):
        for BK in (4, 8, 12) if form != GENERAL else (4, 8):
            for rows in (False, True) if BK >= 8 and form != GENERAL else (False,):
                for wcap in (8, 12, 16) if R == 4 and BK >= 8 else (16,):
                    out.append(("sweep", R, form, BK, rows, wcap))
    return out


TABLE = ([e for form in (PLAIN, COLW, GENERAL) for e in _sweep_entries(form)]
         + [("post", form, BK) for form in (PLAIN, COLW, GENERAL) for BK in ((4, 8, 12) if form != GENERAL else (4, 8))]
         + [("tail", R, form) for R in (1, 2, 4) for form in (PLAIN, COLW, GENERAL)]
         + [("log", R, W, mod) for R, W in LOG_SHAPES for mod in (False, True)])

# the entries that NO call reaches on the release library (no lab switch): see test_release_rule_reaches
LAB_ONLY = {
    # Four cells per lane start at 1921 bases = 8 chunk waves; with the row maker that is nine waves, class 12.  Class 8 WITH a
    # row maker is W <= 7, below 1793 bases: TK_CRF_BAND_R = 4 only.  (Without one it is exactly W = 8 on rows wider than the
    # row image -- S > 48: the plain CRF at nbase 5, cat-mod from five modifications on -- and the general form: reached.  The
    # feed without a row maker at one and two cells per lane is reached the same way.)
    ("sweep", 4, PLAIN, 8, True, 8), ("sweep", 4, PLAIN, 12, True, 8), ("sweep", 4, COLW, 8, True, 8), ("sweep", 4, COLW, 12, True, 8),
}


def _entry_name(e):
    if e[0] == "sweep":
        return "sweep<R %d, %s, BK %d, %s, WCAP %d>" % (e[1], FORM_NAMES[e[2]], e[3], "rows" if e[4] else "self", e[5])
    if e[0] == "post":
        return "posterior<%s, BK %d>" % (FORM_NAMES[e[1]], e[2])
    if e[0] == "tail":
        return "tail<R %d, %s>" % (e[1], FORM_NAMES[e[2]])
    return "crf_kernel<%d, %d, %s>" % (e[1], e[2], "cat-mod" if e[3] else "plain")


# ---------------------------------------------------------------------------------------------------------------------
# the rules, restated
# ---------------------------------------------------------------------------------------------------------------------
PLAN_FIELDS = ("log_domain", "log_R", "log_W", "log_CK", "R", "W", "BK", "bias2", "slope", "rows", "wcap", "retry_BK", "retry_bias2",
               "retry_slope", "retry_R", "retry_W", "side_by_side", "tail_log_R", "slots", "tail_R")
F32 = np.float32


def crf_pick_shape(L):
    if L <= WAVE:
        return 1, 1
    W = 1
    while 2 * W * WAVE < L and W < 16:
        W *= 2
    R = 2
    while R * W * WAVE < L:
        R *= 2
    return R, W


def crf_ck(R, W, kinds):
    c = 28672 // (R * W * WAVE * (kinds + 1))
    return 16 if c >= 16 else 8 if c >= 8 else 4 if c >= 4 else 2


def crf_band_pick_R(L, mod, env):
    R = 2 if not mod and L > 8 * WAVE else 1
    if "TK_CRF_BAND_R" in env:
        R = int(env["TK_CRF_BAND_R"])
        R = R if R in (1, 2, 4) else 1
    while R < 4 and R * WAVE * (MAXW - 1) < L:
        R *= 2
    return R


def crf_band_pick_block(sharp, mod, L, colw, nblk, bulk, env):
    """(bk, bias, slope); the comparisons with the sharpening factor are float32's."""
    x = F32(sharp) if sharp > 0 else F32(1)
    narrow = nblk > 0 and float(bulk) > (0.62 if mod else 0.78) * float(nblk)
    if x <= F32(1.03) and mod and nblk > 0 and float(bulk) > 0.78 * float(nblk):
        b = [4, 0.0, 20]
    elif x <= F32(1.03) and narrow and (not mod or colw):
        b = [8, 3.0, 11]
    elif not mod and x <= F32(1.03):
        b = [12, 3.0, KLIP]
    elif mod and colw and x <= F32(1.03) and L > 11 * WAVE:
        b = [12, 3.0, KLIP]
    elif x <= F32(1.36):
        b = [8, 0.0, KLIP]
    elif x <= F32(1.76):
        b = [8, 3.0, KLIP]
    elif x <= F32(3.5):
        b = [4, 0.0, KLIP]
    else:
        b = [0, 0.0, KLIP]
    if "TK_CRF_BK" in env:
        v = int(env["TK_CRF_BK"])
        if v in (4, 8) or (v == 12 and (not mod or colw)):
            b[0] = v
    if "TK_CRF_WBIAS" in env:
        b[1] = float(env["TK_CRF_WBIAS"])
    if "TK_CRF_KLIP" in env:
        b[2] = int(env["TK_CRF_KLIP"])
    return tuple(b)


def crf_band_pick_retry(sharp, fast, env):
    x = F32(sharp) if sharp > 0 else F32(1)
    if fast[0] == 0 or x > F32(3.5) or "TK_CRF_NO_RETRY" in env:
        return (0, 0.0, KLIP)
    g = F32(7.2) * x
    bias, klip = F32(0), 20
    if g + F32(20) > F32(31.4):
        need = np.ceil(F32(2) * (g + F32(20) - F32(31.4))) * F32(0.5)
        bmax = np.floor(F32(2) * max(F32(0), F32(30.5) - g)) * F32(0.5)
        bias = min(need, bmax)
        klip = min(20, int(np.floor(F32(31.4) - g + bias)))
    if "TK_CRF_RETRY_KLIP" in env:
        klip = int(env["TK_CRF_RETRY_KLIP"])
    if "TK_CRF_RETRY_WBIAS" in env:
        bias = float(env["TK_CRF_RETRY_WBIAS"])
    if klip <= KLIP or (fast[0] == 4 and fast[2] >= klip):
        return (0, 0.0, KLIP)
    return (4, float(bias), klip)


def crf_band_retry_R(L):
    R = 1
    while R < 4 and R * WAVE * (MAXW // 2) < L:
        R *= 2
    return R


def crf_band_retry_slots(nbatch):
    return min(max((nbatch + 15) // 16, 4), nbatch)


def band_use_rows(W, S, mod, colw, bk, env):
    if bk < 8 or W + 1 > MAXW or (mod and not colw) or S > ROW_PITCH:
        return False
    return env["TK_CRF_FEED"][0] == "r" if "TK_CRF_FEED" in env else True


def band_wave_class(R, bk, nw):
    if R != 4 or bk < 8:
        return MAXW
    return 8 if nw <= 8 else 12 if nw <= 12 else MAXW


def crf_log_lds_bytes(R, W, S, kinds):
    SP, CK, NT = S + 2, crf_ck(R, W, kinds), W * WAVE
    f = CK * SP + CK * kinds * R * NT + max(CK * R * NT, kinds * W * SP + kinds * SP)
    f += 2 * CK + 2 + kinds * (SP + 1) + W * WAVE + 9 * W + 10
    return (f * 4 + 15) // 16 * 16


def plan_rule(ntrans, nblk, nbatch, max_seqlen, bulk, form, want_grad, sharp, env=None):
    """What tk_lab_crf_plan reports for a call whose workspace is the library's own query, under the switches `env`:
    a dict over PLAN_FIELDS, or None where the call is refused."""
    env = env or {}
    mod, colw, kinds = form > 0, form == COLW, 3 if form > 0 else 2
    L = max_seqlen if max_seqlen else nblk + 1
    sh = crf_pick_shape(L)
    if sh[0] * sh[1] * WAVE < L or sh[0] > 4 or ntrans > 62:
        return None
    blk = crf_band_pick_block(sharp, mod, L, colw, nblk, bulk, env)
    band = not (env.get("TK_CRF_MODE", "b")[0] == "c" or blk[0] <= 0 or L > 4 * WAVE * MAXW or env.get("TK_CRF_LATTICE_MB") == "0")
    p = dict.fromkeys(PLAN_FIELDS, 0)
    if not band:
        if crf_log_lds_bytes(sh[0], sh[1], ntrans, kinds) > 160 * 1024:
            return None
        p.update(log_domain=1, log_R=sh[0], log_W=sh[1], log_CK=crf_ck(sh[0], sh[1], kinds), slots=nbatch)
        return p
    rblk = crf_band_pick_retry(sharp, blk, env)
    R, rR = crf_band_pick_R(L, mod, env), crf_band_retry_R(L)
    W = max(1, -(-L // (R * WAVE)))
    rows = band_use_rows(W, ntrans, mod, colw, blk[0], env)
    tail_log_R = 4 if rR == 4 else 2
    p.update(log_R=tail_log_R, log_W=16, log_CK=crf_ck(tail_log_R, 16, kinds), R=R, W=W, BK=blk[0], bias2=int(round(2 * blk[1])),
             slope=blk[2], rows=int(rows), wcap=band_wave_class(R, blk[0], W + int(rows)), tail_log_R=tail_log_R,
             slots=crf_band_retry_slots(nbatch), tail_R=rR)
    if rblk[0] > 0:
        rW = max(1, -(-L // (rR * WAVE)))
        p.update(retry_BK=rblk[0], retry_bias2=int(round(2 * rblk[1])), retry_slope=rblk[2], retry_R=rR, retry_W=rW,
                 side_by_side=int(2 * rW <= MAXW))
    return p


def plan_entries(p, form, want_grad):
    """The table entries a call with plan `p` launches (the tail launch runs behind every band launch; whether it finds a
    read to retry is the case's business)."""
    if p["log_domain"]:
        return {("log", p["log_R"], p["log_W"], form > 0)}
    out = {("sweep", p["R"], form, p["BK"], bool(p["rows"]), p["wcap"]), ("tail", p["tail_R"], form)}
    if want_grad:
        out.add(("post", form, p["BK"]))
    return out


class _Env:
    """The lab switches of `env` in the process environment (and nothing else of TK_CRF_* / TK_CATMOD_*) for a while."""

    def __init__(self, env):
        self.env = dict(env or {})

    def __enter__(self):
        self.saved = {k: v for k, v in os.environ.items() if k.startswith(("TK_CRF_", "TK_CATMOD_", "TK_SEPARATE_"))}
        for k in self.saved:
            del os.environ[k]
        os.environ.update(self.env)

    def __exit__(self, *exc):
        for k in self.env:
            os.environ.pop(k, None)
        os.environ.update(self.saved)


def lab_plan(ntrans, nblk, nbatch, max_seqlen, bulk, form, want_grad, sharp, env=None, workspace_bytes=None):
    """The library's own plan under the switches `env` (tk_lab_crf_plan, the lab library; the workspace: the library's query)."""
    was_lab = _lib.is_lab()
    L = _lib.use_lab(True)
    try:
        with _Env(env):
            if workspace_bytes is None:
                workspace_bytes = L.tk_crf_flipflop_workspace_bytes_sharp(ntrans, nblk, nbatch, max_seqlen, int(want_grad), float(sharp))
            out = (ctypes.c_size_t * 20)()
            if not L.tk_lab_crf_plan(ntrans, nblk, nbatch, max_seqlen, bulk, form, int(want_grad), float(sharp), workspace_bytes, out):
                return None
            return dict(zip(PLAN_FIELDS, (int(v) for v in out)))
    finally:
        _lib.use_lab(was_lab)


# ---------------------------------------------------------------------------------------------------------------------
# the GPU case tables
# ---------------------------------------------------------------------------------------------------------------------
def _ntrans(form):
    return 40 if form == PLAIN else 40 + 4 + sum(MODS)


def _call_args(form, T, Ls, hint, env):
    """(max_seqlen, bulk_seqlen) as taiyaki_amd.ctc hands them to the library: lengths on the host give both; a hint gives
    the maximum and no bulk; the entry points that take index arrays (the general form) take no bulk."""
    from taiyaki_amd import ctc
    if hint is not None:
        return int(hint), 0
    separate = "TK_CATMOD_GENERAL" in env or "TK_SEPARATE_INDEX_BUILD" in env
    return int(max(Ls)), 0 if separate else ctc.bulk_of(np.asarray(Ls))


def _case_env(form, env):
    env = dict(env)
    if form == GENERAL:
        env["TK_CATMOD_GENERAL"] = "1"
    return env


def case_plan(case, want_grad=True, extra_env=None, rule=False):
    env = _case_env(case["form"], dict(case["env"], **(extra_env or {})))
    mx, bulk = _call_args(case["form"], case["T"], case["Ls"], case.get("hint"), env)
    args = (_ntrans(case["form"]), case["T"], len(case["Ls"]), mx, bulk, case["form"], want_grad, 1.0)
    return plan_rule(*args, env=env) if rule else lab_plan(*args, env=env)


# (a) the log-domain kernel on every read
def _log_batches():
    out = []
    lo = {sh: 1 if k == 0 else LOG_SHAPES[k - 1][0] * LOG_SHAPES[k - 1][1] * WAVE + 1 for k, sh in enumerate(LOG_SHAPES)}
    for sh in LOG_SHAPES:
        cap = sh[0] * sh[1] * WAVE
        tops = [("cap", cap)] + ([("first", lo[sh])] if sh != (1, 1) else []) + ([("second", lo[sh] + 1)] if sh in ((2, 1), (2, 4), (2, 8), (2, 16)) else [])
        for which, top in tops:
            T = top - 1                                     # the longest read is L = T + 1
            Ls = [top] + [L for L in (1, 64, 65) if L < top] + [top // 2 + 3]
            for form in (PLAIN, COLW):
                out.append(dict(id="log-%dx%d-%s-%s" % (sh + (which, "catmod" if form else "plain")), form=form, T=T, Ls=tuple(Ls[:5]),
                                env={"TK_CRF_MODE": "ckpt"}, want=("log",) + sh + (form > 0,), kind="iid", seed=2700 + top + form))
    return out


LOG_CASES = _log_batches()


# (b) the linear path.  Per (form kind, R): one input whose reads end one before, on and one after a chunk boundary and in the third
# chunk wave; iid scores, L <= 0.7 T for the plain CRF, L ~ T / 2 for cat-mod on normalised columns.  T mod 4, 8, 12 != 0.
BAND_T = {(False, 1): 203, (False, 2): 383, (False, 4): 751, (True, 1): 269, (True, 2): 523, (True, 4): 1037}
BAND_BIAS = {4: "0", 8: "0", 12: "3"}
CLASS_HINT = {8: None, 12: 2500, 16: 3500}     # four cells per lane: W = 3 (the reads' own), 10, 14 chunk waves -- the same class with and without the row maker


def _band_batches():
    out = []
    for form in (PLAIN, COLW, GENERAL):
        for R in (1, 2, 4):
            PW = R * WAVE
            for BK in (4, 8, 12) if form != GENERAL else (4, 8):
                for wcap in (8, 12, 16) if R == 4 and BK >= 8 else (16,):
                    feeds = ("rows", "self") if BK >= 8 and form != GENERAL else ("self",)
                    env = {"TK_CRF_MODE": "band", "TK_CRF_BAND_R": str(R), "TK_CRF_BK": str(BK), "TK_CRF_WBIAS": BAND_BIAS[BK]}
                    out.append(dict(id="band-%s-r%d-bk%d-w%d" % (("plain", "colw", "general")[form], R, BK, wcap), form=form,
                                    T=BAND_T[(form > 0, R)], Ls=(PW - 1, PW, PW + 1, 2 * PW + 5, 1, 2 * PW), env=env,
                                    hint=CLASS_HINT[wcap] if R == 4 and BK >= 8 else None, feeds=feeds,
                                    want=[("sweep", R, form, BK, feed == "rows", wcap) for feed in feeds], kind="iid",
                                    seed=2750 + R + 10 * (form > 0)))
    return out


BAND_CASES = _band_batches()

# ... and each wave-count class once per form with a read in the class's top wave (four cells per lane: 256 cells a wave).  The
# plain CRF and cat-mod with per-column factors on iid scores with L <= 0.7 T (normalised modification columns; the 12-step
# blocks the release rule gives cat-mod from 705 bases on disown every read of these batches on synth.confident_scores --
# non-finite sweep scores; the retry keeps them: LABNOTES), the general form at its 8-step blocks on confident scores.
HEAVY_CASES = [
    dict(id="heavy-plain-w8", form=PLAIN, T=2453, Ls=(1700, 1535, 1536, 1537), env={"TK_CRF_MODE": "band", "TK_CRF_BAND_R": "4"}, hint=1700, top=7,
         want=("sweep", 4, PLAIN, 12, True, 8), kind="iid", seed=2781),
    dict(id="heavy-plain-w12", form=PLAIN, T=3901, Ls=(2700, 2559, 2560, 2561), env={}, hint=2700, top=11,
         want=("sweep", 4, PLAIN, 12, True, 12), kind="iid", seed=2782),
    dict(id="heavy-plain-w16", form=PLAIN, T=4153, Ls=(2900, 2815, 2816, 2817), env={}, hint=2900, top=12,
         want=("sweep", 4, PLAIN, 12, True, 16), kind="iid", seed=2783),
    dict(id="heavy-colw-w8", form=COLW, T=2453, Ls=(1700, 1535, 1536, 1537), env={"TK_CRF_MODE": "band", "TK_CRF_BAND_R": "4"}, hint=1700, top=7,
         want=("sweep", 4, COLW, 12, True, 8), kind="iid", seed=2784),
    dict(id="heavy-general-w8", form=GENERAL, T=2861, Ls=(2000, 1791, 1792, 1793), env={"TK_CRF_MODE": "band", "TK_CRF_BAND_R": "4"}, hint=2000, top=8,
         want=("sweep", 4, GENERAL, 8, False, 8), kind="confident", seed=2789),
    dict(id="heavy-colw-w12", form=COLW, T=3901, Ls=(2700, 2559, 2560, 2561), env={}, hint=2700, top=11,
         want=("sweep", 4, COLW, 12, True, 12), kind="iid", seed=2785),
    dict(id="heavy-colw-w16", form=COLW, T=4153, Ls=(2900, 2815, 2816, 2817), env={}, hint=2900, top=12,
         want=("sweep", 4, COLW, 12, True, 16), kind="iid", seed=2786),
    dict(id="heavy-general-w12", form=GENERAL, T=3901, Ls=(2900, 2815, 2816, 2817), env={}, hint=2900, top=12,
         want=("sweep", 4, GENERAL, 8, False, 12), kind="confident", seed=2786 + 1),
    dict(id="heavy-general-w16", form=GENERAL, T=4153, Ls=(3100, 3071, 3072, 3073), env={}, hint=3100, top=13,
         want=("sweep", 4, GENERAL, 8, False, 16), kind="confident", seed=2788),
]

# (c) the tail launch: two ordinary reads, bands of 2, 5, 8 and 12 cells (L = T + 2 - width: under iid scores the fast
# configuration disowns them and, from T ~ 500 on, so does the retry -- crf_read's reads) and reads of 0.91, 0.94 and 0.97 T (bands
# of 3 - 9 % of T: the fast configuration disowns most of them, the retry keeps them); the lengths carry their maximum and no
# bulk; nine reads share four slots.  The retry's cells per lane by the longest read: 1 (<= 512), 2 (<= 1024), 4; beyond 2048
# its sweeps run one after the other.
TAIL_T = {"r1": 505, "r2": 1003, "r4": 1501, "r4seq": 2101}


def _tail_batches():
    out = []
    for rng_, T in TAIL_T.items():
        Ls = (T, T // 2 + 7, T - 3, int(0.94 * T), T - 6, T // 3 + 1, T - 10, int(0.97 * T), int(0.91 * T))
        for form in (PLAIN, COLW, GENERAL):
            out.append(dict(id="tail-%s-%s" % (rng_, ("plain", "colw", "general")[form]), form=form, T=T, Ls=Ls, env={}, hint=max(Ls),
                            want=("tail", {"r1": 1, "r2": 2}.get(rng_, 4), form), side_by_side=rng_ != "r4seq", kind="iid",
                            seed=2790 + T % 7))
    return out


TAIL_CASES = _tail_batches()

# Cases whose gradient is held to parity.crf_grad_ok (which allows the reference's own noise) instead of GRAD_T_ATOL from the
# witness alone: {case id: (measured distance from float64, the reference's own)}.  None needed it when this was written.
NOISE_ALLOWED = {}


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the table, the rules, the coverage
# ---------------------------------------------------------------------------------------------------------------------
def test_table_has_85_entries():
    kinds = [e[0] for e in TABLE]
    assert len(TABLE) == len(set(TABLE)) == 85
    assert (kinds.count("sweep"), kinds.count("post"), kinds.count("tail"), kinds.count("log")) == (54, 8, 9, 14)
    assert [len(_sweep_entries(f)) for f in (PLAIN, COLW, GENERAL)] == [23, 23, 8]
    assert LAB_ONLY <= set(TABLE)


def test_checkpoint_spacing_of_every_log_domain_shape():
    """crf_ck: 16, 8, 4, 2 -- and at (4, 16) cat-mod the quotient is 1, the spacing is clamped to 2 and the LDS image is
    137 KB (136784 bytes at S = 46), above the 112 KiB the formula aims at and below the 160 KiB a workgroup has."""
    assert [(crf_ck(R, W, 2), crf_ck(R, W, 3)) for R, W in LOG_SHAPES] == [(16, 16), (16, 16), (16, 16), (16, 8), (8, 4), (4, 2), (2, 2)]
    assert 28672 // (4 * 16 * WAVE * 4) == 1
    assert 136000 < crf_log_lds_bytes(4, 16, 46, 3) < 138000 and crf_log_lds_bytes(4, 16, 62, 3) <= 160 * 1024
    for R, W in LOG_SHAPES[:-1]:
        assert crf_log_lds_bytes(R, W, 62, 3) <= 115 * 1024 and crf_log_lds_bytes(R, W, 62, 2) <= 115 * 1024


LENGTHS = sorted({L + d for L in (64, 128, 256, 512, 704, 960, 1024, 1792, 1920, 2048, 2816, 3072, 3840, 4096) for d in (0, 1)} | {1, 2, 63, 300, 3000})
SHARPS = [1.0, 1.03, 1.0301, 1.36, 1.3601, 1.58, 1.59, 1.76, 1.7601, 2.8, 3.0, 3.5, 3.5001, 5.0]


def _grid():
    for form, S in ((PLAIN, 40), (PLAIN, 48), (PLAIN, 60), (COLW, 46), (COLW, 48), (COLW, 49), (GENERAL, 46), (GENERAL, 49)):
        for L in LENGTHS:
            nblk = max(L - 1, int(L / 0.8), 1)
            # the bulk on both sides of 0.62 T and 0.78 T, and unknown
            for bulk in (0, int(0.62 * nblk), int(0.62 * nblk) + 1, int(0.78 * nblk), int(0.78 * nblk) + 1):
                if bulk > L:
                    continue
                for sharp in SHARPS:
                    yield S, nblk, L, bulk, form, sharp


def test_plan_rule_is_the_librarys_around_every_threshold():
    seen = set()
    L_ = _lib.use_lab(True)
    try:
        with _Env({}):
            out = (ctypes.c_size_t * 20)()
            for S, nblk, L, bulk, form, sharp in _grid():
                for g in (1, 0):
                    wsb = L_.tk_crf_flipflop_workspace_bytes_sharp(S, nblk, 5, L, g, sharp)
                    got = dict(zip(PLAN_FIELDS, (int(v) for v in out))) if L_.tk_lab_crf_plan(S, nblk, 5, L, bulk, form, g, sharp, wsb, out) else None
                    want = plan_rule(S, nblk, 5, L, bulk, form, g, sharp)
                    assert got == want, ((S, nblk, L, bulk, form, g, sharp), got, want)
                    seen |= plan_entries(got, form, g) if got is not None else set()
            # refused: no instantiation beyond 4096 bases in the log domain, no workspace, no such form
            assert not L_.tk_lab_crf_plan(40, 9000, 5, 4097, 0, 0, 1, 5.0, 1 << 40, out) and plan_rule(40, 9000, 5, 4097, 0, 0, 1, 5.0) is None
            assert not L_.tk_lab_crf_plan(40, 9000, 5, 4097, 0, 0, 1, 1.0, 1 << 40, out)
            assert not L_.tk_lab_crf_plan(40, 300, 5, 200, 0, 0, 1, 1.0, 0, out) and not L_.tk_lab_crf_plan(40, 300, 5, 200, 0, 3, 1, 1.0, 1 << 30, out)
            assert not L_.tk_lab_crf_plan(63, 300, 5, 200, 0, 0, 1, 1.0, 1 << 30, out)
            # a workspace that holds the batch's layout and not the retry's: no retry; the log-domain form's alone: that form
            full = L_.tk_crf_flipflop_workspace_bytes_sharp(40, 300, 64, 200, 1, 1.0)
            assert L_.tk_lab_crf_plan(40, 300, 64, 200, 0, 0, 1, 1.0, full, out) and (out[0], out[11]) == (0, 4)
            log_only = L_.tk_crf_flipflop_workspace_bytes_sharp(40, 300, 64, 200, 1, 5.0)
            assert log_only < full and L_.tk_lab_crf_plan(40, 300, 64, 200, 0, 0, 1, 1.0, log_only, out) and out[0] == 1
    finally:
        _lib.use_lab(False)
    # slots, the max_seqlen default
    assert [crf_band_retry_slots(n) for n in (1, 3, 4, 5, 64, 65, 80, 81)] == [1, 3, 4, 4, 4, 5, 5, 6]
    assert plan_rule(40, 300, 5, 0, 0, 0, 1, 1.0) == plan_rule(40, 300, 5, 301, 0, 0, 1, 1.0) == lab_plan(40, 300, 5, 0, 0, 0, 1, 1.0)
    assert lab_plan(40, 300, 81, 200, 0, 0, 1, 1.0)["slots"] == 6
    assert seen <= set(TABLE)


def test_plan_rule_is_the_librarys_under_every_lab_switch():
    """The switches the GPU cases set: cells per lane, block length, bias, feed, the form, no retry, the workspace cap."""
    for form, S in ((PLAIN, 40), (COLW, 46), (GENERAL, 46)):
        for R, BK, feed, L in itertools.product((1, 2, 4), (4, 8, 12), ("rows", "self"), (133, 300, 960, 961, 1792, 1793, 2048, 2049, 2500, 2816, 2817, 3072, 3073, 3500, 3840, 3841, 4096)):
            env = {"TK_CRF_MODE": "band", "TK_CRF_BAND_R": str(R), "TK_CRF_BK": str(BK), "TK_CRF_WBIAS": BAND_BIAS[BK], "TK_CRF_FEED": feed}
            args = (S, 1200, 6, L, 0, form, 1, 1.0)
            assert lab_plan(*args, env=env) == plan_rule(*args, env=env), (args, env)
        for env in ({"TK_CRF_MODE": "ckpt"}, {"TK_CRF_LATTICE_MB": "0"}, {"TK_CRF_NO_RETRY": "1"}, {"TK_CRF_NO_FALLBACK": "1"},
                    {"TK_CRF_KLIP": "11"}, {"TK_CRF_RETRY_KLIP": "18", "TK_CRF_RETRY_WBIAS": "1.5"}, {"TK_CRF_BAND_R": "3"}):
            for L in LENGTHS:
                for g in (1, 0):
                    args = (S, max(L, 100), 7, L, 0, form, g, 1.0)
                    assert lab_plan(*args, env=env) == plan_rule(*args, env=env), (args, env)


def test_release_rule_reaches():
    """Which of the 85 entries a call can reach on the release library -- every form, alphabet width, length, bulk and
    sharpening factor of the threshold grid -- and which only a lab switch reaches: LAB_ONLY, candidates for removal."""
    seen = set()
    for S, nblk, L, bulk, form, sharp in _grid():
        for g in (1, 0):
            p = plan_rule(S, nblk, 5, L, bulk, form, g, sharp)
            if p is not None:
                seen |= plan_entries(p, form, g)
    assert seen <= set(TABLE)
    assert set(TABLE) - seen == LAB_ONLY, sorted(set(TABLE) - seen - LAB_ONLY) + sorted(LAB_ONLY - (set(TABLE) - seen))


def test_case_tables_reach_every_entry():
    reached = set()
    for case in LOG_CASES:
        for g in (True, False):
            p = case_plan(case, g)
            assert p == case_plan(case, g, rule=True) and plan_entries(p, case["form"], g) == {case["want"]}, case["id"]
            assert p["log_CK"] == crf_ck(case["want"][1], case["want"][2], 3 if case["form"] else 2)
        reached.add(case["want"])
        assert max(case["Ls"]) == case["T"] + 1 and 1 in case["Ls"] and 3 <= len(case["Ls"]) <= 5, case["id"]
    # T mod CK takes 0, 1 and CK - 1 at every spacing
    for ck in (16, 8, 4, 2):
        res = {c["T"] % ck for c in LOG_CASES if crf_ck(c["want"][1], c["want"][2], 3 if c["form"] else 2) == ck}
        assert {0, 1, ck - 1} <= res, (ck, res)
    for case in BAND_CASES:
        PW = case["want"][0][1] * WAVE
        for feed, want in zip(case["feeds"], case["want"]):
            p = case_plan(case, True, {"TK_CRF_FEED": feed})
            assert p == case_plan(case, True, {"TK_CRF_FEED": feed}, rule=True), case["id"]
            assert plan_entries(p, case["form"], True) >= {want, ("post", case["form"], want[3])}, (case["id"], p)
            reached |= {want, ("post", case["form"], want[3])}
        assert all(case["T"] % bk for bk in (4, 8, 12)) and {PW - 1, PW, PW + 1} <= set(case["Ls"]), case["id"]
        if case["hint"] is None:
            assert -(-max(case["Ls"]) // PW) == p["W"] == 3, case["id"]         # a read in the launch's top chunk wave
    for case in HEAVY_CASES:
        p = case_plan(case)
        assert p == case_plan(case, rule=True) and case["want"] in plan_entries(p, case["form"], True), (case["id"], p)
        assert p["W"] == case["top"] == -(-max(case["Ls"]) // 256) and all(case["T"] % bk for bk in (4, 8, 12)), case["id"]
        k = sorted(case["Ls"])[1]
        assert k % 256 == 0 and {k - 1, k, k + 1} <= set(case["Ls"]), case["id"]
        # the class's top wave: with one chunk wave more the launch would be the next class's
        nw = p["W"] + p["rows"]
        assert band_wave_class(4, p["BK"], nw) == case["want"][5] and (case["want"][5] == 16 or band_wave_class(4, p["BK"], nw + 1) > case["want"][5])
        reached.add(case["want"])
    for f in (PLAIN, COLW, GENERAL):
        assert {c["want"][5] for c in HEAVY_CASES if c["form"] == f} == {8, 12, 16}
    for case in TAIL_CASES:
        for g in (True, False):
            p = case_plan(case, g)
            assert p == case_plan(case, g, rule=True) and case["want"] in plan_entries(p, case["form"], g), (case["id"], p)
            assert p["retry_BK"] == 4 and p["retry_R"] == case["want"][1] and bool(p["side_by_side"]) == case["side_by_side"], (case["id"], p)
            assert p["tail_log_R"] == (4 if case["want"][1] == 4 else 2)
            assert case_plan(case, g, {"TK_CRF_NO_RETRY": "1"})["retry_BK"] == 0
        widths = sorted(case["T"] + 2 - L for L in case["Ls"])
        assert widths[:4] == [2, 5, 8, 12] and widths[4] > 12 and p["slots"] == 4 < len(case["Ls"]), case["id"]
        reached.add(case["want"])
    assert {c["side_by_side"] for c in TAIL_CASES if c["want"][1] == 4} == {True, False}
    assert reached == set(TABLE), sorted(set(TABLE) - reached)
    ids = [c["id"] for c in LOG_CASES + BAND_CASES + HEAVY_CASES + TAIL_CASES]
    assert len(ids) == len(set(ids)) and set(NOISE_ALLOWED) <= set(ids)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
ORACLE_MAX_T = 1100


@functools.lru_cache(maxsize=3)
def _inputs(form_is_mod, T, Ls, kind, seed):
    """The input of a case with its references beside it, computed once: the float64 witness always, the C oracle where
    T <= 1100 (its time grows with T x L)."""
    import oracle
    inp = synth.crf_case(T, len(Ls), seed, seqlens=np.array(Ls, dtype=np.int32), nmods_per_base=MODS if form_is_mod else None)
    if kind == "confident":
        synth.confident_scores(inp, seed + 1)
    if form_is_mod:
        synth.normalise_mod_columns(inp, logit_scale=0.2)
    wloss, wgrad = parity.oracle_crf_f64(oracle, inp, 1.0)
    oloss = ograd = None
    if T <= ORACLE_MAX_T:
        oloss, ograd = parity.oracle_crf(oracle, inp, 1.0)
    return inp, wloss, wgrad, oloss, ograd


def _case_inputs(case):
    return _inputs(case["form"] > 0, case["T"], tuple(case["Ls"]), case["kind"], case["seed"])


def _run(case, dev, want_grad, env, labenv, poisoned=False):
    """One call of the operator under the case's switches: (loss, gradient or None, reads retried, reads redone)."""
    import torch
    from taiyaki_amd import ctc
    inp = _case_inputs(case)[0]
    env = _case_env(case["form"], dict(case["env"], **env))
    for k in ("TK_CRF_MODE", "TK_CRF_BAND_R", "TK_CRF_BK", "TK_CRF_WBIAS", "TK_CRF_FEED", "TK_CATMOD_GENERAL", "TK_CRF_NO_RETRY", "TK_CRF_NO_FALLBACK"):
        labenv.delenv(k)
    for k, v in env.items():
        labenv.setenv(k, v)
    if not env:
        _lib.use_lab(False)
    assert _lib.is_lab() == bool(env) and _lib.is_strict()
    assert not _FAILED_LAUNCH, "an earlier launch of this module failed: nothing more is launched"
    try:
        return _launch(case, inp, dev, want_grad, poisoned)
    except RuntimeError:
        _FAILED_LAUNCH.append(case["id"])
        raise


_FAILED_LAUNCH = []


def _launch(case, inp, dev, want_grad, poisoned):
    import torch
    from taiyaki_amd import ctc
    if not poisoned:
        loss, grad = parity.run_crf(inp, 1.0, dev, want_grad=want_grad, max_seqlen=case.get("hint"))
        return loss, grad, ctc.last_retry_count(), ctc.last_gate_count()
    x = torch.from_numpy(inp["scores"]).to(dev)
    seqs, sl = torch.from_numpy(inp["seqs"]), ctc.set_max_seqlen(torch.from_numpy(inp["seqlens"]), case["hint"])
    extra = (torch.from_numpy(inp["mod_cats"]), inp["can_mods_offsets"], inp["mod_cat_weights"]) if case["form"] else ()
    # the caching allocator hands these blocks out for the outputs: the gradient's, and NaN for every small block (the costs come
    # after the call's index buffers)
    junk = [torch.full_like(x, float("nan"))] + [torch.full((128,), float("nan"), device=dev) for _ in range(256)]
    del junk
    c, g = ctc._run(x, seqs, sl, 1.0, 1.0, 1.0, 40, want_grad, *extra)
    torch.cuda.synchronize()
    return c.cpu().numpy(), g.cpu().numpy() if want_grad else None, ctc.last_retry_count(), ctc.last_gate_count()


def _figures(case, loss, grad):
    """Per read: the loss criterion; over the batch: the gradient's distance from the witness and from the oracle on the
    posterior scale, the oracle's own distance from the witness."""
    inp, wloss, wgrad, oloss, ograd = _case_inputs(case)
    T = case["T"]
    ps = parity.posterior_scale(inp) * T
    fig = dict(loss_f64_rel=parity.rel_err(loss, wloss), finite=bool(np.isfinite(loss).all() and (grad is None or np.isfinite(grad).all())))
    ok_w = parity.crf_loss_ok(dict(loss=loss, oloss=wloss))
    fig["loss_ok"] = bool(ok_w or (oloss is not None and parity.crf_loss_ok(dict(loss=loss, oloss=oloss))))
    fig["loss_rel"] = parity.rel_err(loss, oloss) if oloss is not None else float("nan")
    if grad is not None:
        fig["grad_f64_scaled"] = parity.abs_err(grad * ps, wgrad * ps)
        fig["grad_scaled_abs"] = parity.abs_err(grad * ps, ograd * ps) if ograd is not None else float("nan")
        fig["ref_noise_scaled"] = parity.abs_err(ograd * ps, wgrad * ps) if ograd is not None else float("nan")
    return fig


def _line(case, what, entry, fig, retried, redone, note=""):
    print("r27| %-26s %-9s %-58s loss vs oracle %8.2e vs f64 %8.2e | grad vs oracle %8.2e vs f64 %8.2e (oracle's own %8.2e) | retried %d redone %d%s"
          % (case["id"], what, _entry_name(entry), fig["loss_rel"], fig["loss_f64_rel"], fig.get("grad_scaled_abs", float("nan")),
             fig.get("grad_f64_scaled", float("nan")), fig.get("ref_noise_scaled", float("nan")), retried, redone, note))


def _assert_parity(case, fig, want_grad):
    assert fig["finite"] and fig["loss_ok"], (case["id"], fig)
    if not want_grad:
        return
    if case["id"] in NOISE_ALLOWED:
        assert fig["ref_noise_scaled"] == fig["ref_noise_scaled"] and parity.crf_grad_ok(fig), (case["id"], fig)
    else:
        assert fig["grad_f64_scaled"] < parity.GRAD_T_ATOL, (case["id"], fig)


@pytest.mark.gpu
@pytest.mark.parametrize("case", LOG_CASES, ids=lambda c: c["id"])
def test_log_domain_kernel_every_shape(gpu_device, labenv, case):
    """(a): crf_kernel<R, W, MOD> on every read of the batch, with a gradient and cost only."""
    entry = case["want"]
    for want_grad in (True, False):
        assert plan_entries(case_plan(case, want_grad), case["form"], want_grad) == {entry}
        loss, grad, retried, redone = _run(case, gpu_device, want_grad, {}, labenv)
        fig = _figures(case, loss, grad)
        _line(case, "grad" if want_grad else "cost", entry, fig, retried, redone, " | T mod CK %d of %d" % (case["T"] % crf_ck(entry[1], entry[2], 3 if entry[3] else 2), crf_ck(entry[1], entry[2], 3 if entry[3] else 2)))
        _assert_parity(case, fig, want_grad)
        assert retried == 0 and redone == 0


def _band_case(case, dev, labenv, feeds, wants):
    out = {}
    for feed, want in zip(feeds, wants):
        extra = {"TK_CRF_FEED": feed} if feed else {}
        p = case_plan(case, True, extra)
        assert want in plan_entries(p, case["form"], True) and ("post", case["form"], want[3]) in plan_entries(p, case["form"], True), (case["id"], p)
        loss, grad, retried, redone = _run(case, dev, True, extra, labenv)
        fig = _figures(case, loss, grad)
        _line(case, "grad", want, fig, retried, redone, " | bias %.1f slope %d W %d" % (p["bias2"] / 2, p["slope"], p["W"]))
        # nobody else's answer: every read stayed on the linear path of THIS instantiation
        assert retried == 0 and redone == 0, (case["id"], feed, retried, redone)
        _assert_parity(case, fig, True)
        out[feed] = (loss, grad)
    if len(out) == 2:
        (l0, g0), (l1, g1) = out.values()
        assert np.array_equal(l0, l1) and np.array_equal(g0, g1), (case["id"], "the two feeds differ")


@pytest.mark.gpu
@pytest.mark.parametrize("case", BAND_CASES, ids=lambda c: c["id"])
def test_linear_path_every_sweep_and_gradient_pass(gpu_device, labenv, case):
    """(b): crf_band_sweep_kernel and crf_band_posterior_kernel, every instantiation; nothing retried, nothing redone."""
    _band_case(case, gpu_device, labenv, case["feeds"], case["want"])


@pytest.mark.gpu
@pytest.mark.parametrize("case", HEAVY_CASES, ids=lambda c: c["id"])
def test_linear_path_top_wave_of_every_wave_class(gpu_device, labenv, case):
    """(b): four cells per lane with a read in the top chunk wave of each wave-count class (7 + 1, 11 + 1 and 12 + 1 waves
    with the row maker; 8, 12 and 13 without), the release rule's configuration."""
    _band_case(case, gpu_device, labenv, (None,), (case["want"],))


@pytest.mark.gpu
@pytest.mark.parametrize("case", TAIL_CASES, ids=lambda c: c["id"])
def test_tail_launch_every_instantiation(gpu_device, labenv, case):
    """(c): crf_band_tail_kernel<R, MOD, CW>: the retry, crf_read behind it, and neither."""
    entry, kept_any = case["want"], False
    for want_grad in (True, False):
        what = "grad" if want_grad else "cost"
        p = case_plan(case, want_grad)
        assert entry in plan_entries(p, case["form"], want_grad) and p["retry_R"] == entry[1], (case["id"], p)
        # as shipped
        loss, grad, retried, redone = _run(case, gpu_device, want_grad, {}, labenv)
        fig = _figures(case, loss, grad)
        _line(case, what, entry, fig, retried, redone, " | as shipped, retry W %d %s" % (p["retry_W"], "side by side" if p["side_by_side"] else "one after the other"))
        _assert_parity(case, fig, want_grad)
        assert retried >= 1 and redone <= retried, (case["id"], retried, redone)
        # no retry: crf_read redoes every disowned read
        loss2, grad2, retried2, redone2 = _run(case, gpu_device, want_grad, {"TK_CRF_NO_RETRY": "1"}, labenv)
        fig2 = _figures(case, loss2, grad2)
        _line(case, what, entry, fig2, retried2, redone2, " | no retry: crf_read<%d, 16>" % p["tail_log_R"])
        _assert_parity(case, fig2, want_grad)
        assert retried2 == 0 and redone2 == retried >= 1, (case["id"], retried, redone2)
        # no fallback, outputs poisoned: what the linear path owns is already the shipped run's bits
        loss3, grad3, retried3, redone3 = _run(case, gpu_device, want_grad, {"TK_CRF_NO_FALLBACK": "1"}, labenv, poisoned=True)
        # (a read the linear path disowned twice keeps its poison or what the attempts left there -- the retry's gradient pass
        # may have written every row before it saw one lose mass --, never crf_read's bits)
        own = np.isfinite(loss3) & (loss3 == loss)
        if want_grad:
            own &= np.isfinite(grad3).all(axis=(0, 2)) & (grad3 == grad).all(axis=(0, 2))
        assert retried3 == retried and redone3 == 0 and int(own.sum()) == len(case["Ls"]) - redone, (case["id"], retried3, redone3, own)
        print("r27| %-26s %-9s no fallback: %d of %d reads owned by the linear path, %d of them by the retry; bit-equal to the shipped run"
              % (case["id"], what, int(own.sum()), len(case["Ls"]), retried - redone))
        kept_any = kept_any or retried - redone >= 1
    assert kept_any, (case["id"], "the retry kept no read")
