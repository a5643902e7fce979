"""float64 numpy restatement of the reference squiggle match (taiyaki/squiggle_match/c_squiggle_match.c),
one read at a time, for tests/test_squiggle_match.py.  Test infrastructure only; line numbers cite
c_squiggle_match.c.

Arrays per read: params (npos, 3) = level, log-scale, move logit; signal (nsample,).
"""
import numpy as np

LARGE = 1e30                # :7 LARGE_VAL
LARGE_LOG_VAL = 50000.0     # taiyaki/constants.py (localpen / minscore = None)
LN_HALF = np.log(0.5)


def tables(params, back_prob):
    """loc, logsc, sc, move_pen, stay_pen (:124-130, :474-477)."""
    p = np.asarray(params, dtype=np.float64)
    loc, logsc, logit = p[:, 0], p[:, 1], p[:, 2]
    mp = (1.0 - back_prob) * 0.5 * (1.0 + np.tanh(logit / 2.0))
    return loc, logsc, np.exp(logsc), np.log(mp), np.log1p(-mp - back_prob)


def loglaplace(x, loc, sc, logsc):
    """:10-12"""
    return -np.abs(x - loc) / sc - logsc - np.log(2.0)


def forward(params, signal, back_prob):
    """Forward lattice (nsample + 1, 2, npos): [:, 0] positions, [:, 1] back states (:108-186)."""
    loc, logsc, sc, mpen, spen = tables(params, back_prob)
    npos, lnpb = len(loc), np.log(back_prob)
    f = np.full((len(signal) + 1, 2, npos), -LARGE)
    f[0, 0, 0] = 0.0
    for s, x in enumerate(np.asarray(signal, dtype=np.float64)):
        fp, fb = f[s]
        p = fp + spen
        b = fb + LN_HALF
        p[1:] = np.logaddexp(p[1:], fp[:-1] + mpen[1:])
        b[:-1] = np.logaddexp(b[:-1], fp[1:] + lnpb)
        p[1:] = np.logaddexp(p[1:], fb[:-1] + LN_HALF)
        em = loglaplace(x, loc, sc, logsc)
        f[s + 1, 0], f[s + 1, 1] = p + em, b + em
    return f


def backward(params, signal, back_prob):
    """Backward lattice, same layout (:189-267)."""
    loc, logsc, sc, mpen, spen = tables(params, back_prob)
    npos, lnpb = len(loc), np.log(back_prob)
    n = len(signal)
    g = np.full((n + 1, 2, npos), -LARGE)
    g[n, 0, npos - 1] = 0.0
    sig = np.asarray(signal, dtype=np.float64)
    for s in range(n, 0, -1):
        em = loglaplace(sig[s - 1], loc, sc, logsc)
        tp, tb = g[s, 0] + em, g[s, 1] + em
        p = tp + spen
        p[:-1] = np.logaddexp(p[:-1], tp[1:] + mpen[1:])
        b = tb + LN_HALF
        b[:-1] = np.logaddexp(b[:-1], tp[1:] + LN_HALF)
        p[1:] = np.logaddexp(p[1:], tb[:-1] + lnpb)
        g[s - 1, 0], g[s - 1, 1] = p, b
    return g


def cost(params, signal, back_prob):
    """Negated forward score (:184-185, squiggle_match.pyx:47)."""
    return -forward(params, signal, back_prob)[-1, 0, -1]


def grad(params, signal, back_prob, f=None):
    """Negated gradient (npos, 3) as :591-694 write it: per-sample normaliser over all states; the
    move-logit term without the transition penalty in its exponent (:661-685).  `f`: the forward
    lattice of the same arguments, where the caller has it already."""
    loc, logsc, sc, mpen, spen = tables(params, back_prob)
    f = forward(params, signal, back_prob) if f is None else f
    g = backward(params, signal, back_prob)
    m = 0.5 * (1.0 + np.tanh(np.asarray(params, dtype=np.float64)[:, 2] / 2.0))
    dl = (1.0 - back_prob) * m * (1.0 - m)
    out = np.zeros((len(loc), 3))
    for s in range(1, len(signal) + 1):
        x = float(signal[s - 1])
        post = f[s] + g[s]
        fact = np.logaddexp.reduce(post.ravel())
        w = np.exp(post[0] - fact) + np.exp(post[1] - fact)
        out[:, 0] += w * np.sign(x - loc) / sc
        out[:, 1] += w * (np.abs(x - loc) / sc - 1.0)
        em = loglaplace(x, loc, sc, logsc)
        out[:, 2] -= np.exp(f[s - 1, 0] + g[s, 0] + em - fact) * dl
        out[1:, 2] += np.exp(f[s - 1, 0, :-1] + g[s, 0, 1:] + em[1:] - fact) * dl[1:]
    return -out


def _take(best, code, cand, val):
    """strict '>': a candidate replaces the best so far only when it is larger"""
    better = cand > best
    return np.where(better, cand, best), np.where(better, val, code).astype(np.int8)


def viterbi(params, signal, back_prob, localpen=None, minscore=None, allowed=None):
    """(negated score, path) of :270-454 with its candidate order and strict '>' (first candidate wins a
    tie).  `allowed` (nsample,), a path in the output encoding, restricts every sample to the states
    that path folds onto there (rescoring a path)."""
    localpen = LARGE_LOG_VAL if localpen is None else localpen
    minscore = LARGE_LOG_VAL if minscore is None else minscore
    loc, logsc, sc, mpen, spen = tables(params, back_prob)
    npos, lnpb = len(loc), np.log(back_prob)
    mean_move, mean_stay = mpen.mean(), spen.mean()
    n = len(signal)
    ks = np.arange(npos)
    vs, ve = 0.0, -LARGE
    vp, vb = np.full(npos, -LARGE), np.full(npos, -LARGE)
    # traceback: positions 0 stay, 1 move, 2 from start, 3 from back; back 0 stay, 1 from k + 1; end: -1 stay
    tp = np.zeros((n, npos), dtype=np.int8)
    tbk = np.zeros((n, npos), dtype=np.int8)
    te = np.full(n, -1, dtype=np.int64)
    for s in range(n):
        x = float(signal[s])
        prevp = np.concatenate([[vs], vp[:-1]])
        prevpen = np.concatenate([[mean_move], mpen[:-1]])
        p, code = vp + spen, np.zeros(npos, dtype=np.int8)
        p, code = _take(p, code, prevp + prevpen, 1)
        p, code = _take(p, code, np.where(ks >= 1, vs + mean_move - localpen * ks, -np.inf), 2)
        b, bc = _take(vb + LN_HALF, np.zeros(npos, dtype=np.int8), np.concatenate([vp[1:] + lnpb, [-np.inf]]), 1)
        p, code = _take(p, code, np.concatenate([[-np.inf], vb[:-1] + LN_HALF]), 3)
        ecand = np.concatenate([[ve + mean_stay, vp[-1] + mpen[-1]],
                                vp[:-1] + mpen[:-1] - localpen * (npos - 1 - ks[:-1])])
        k = int(np.argmax(ecand))
        e = ecand[k]
        te[s] = -1 if k == 0 else (npos - 1 if k == 1 else k - 2)
        em = np.maximum(-minscore, loglaplace(x, loc, sc, logsc))
        vp, vb = p + em, b + em
        vs, ve = vs + mean_stay - localpen, e - localpen
        tp[s], tbk[s] = code, bc
        if allowed is not None:
            a = int(allowed[s])
            keep = ks == a
            vp, vb = np.where(keep, vp, -np.inf), np.where(keep, vb, -np.inf)
            if a != -1:
                vs, ve = -np.inf, -np.inf
    score = max(vp[-1], ve)
    cur = ("p", npos - 1) if vp[-1] > ve else ("e", 0)
    path = np.zeros(n, dtype=np.int32)
    for s in range(n - 1, -1, -1):
        kind, k = cur
        path[s] = -1 if kind in "se" else k
        if s == 0:
            break
        if kind == "e":
            cur = ("e", 0) if te[s] < 0 else ("p", int(te[s]))
        elif kind == "b":
            cur = ("p", k + 1) if tbk[s, k] else cur
        elif kind == "p":
            c = tp[s, k]
            cur = {0: cur, 1: ("p", k - 1) if k > 0 else ("s", 0), 2: ("s", 0), 3: ("b", k - 1)}[int(c)]
    return -score, path


def batch(fn, case, *args):
    """Apply a per-read function over a batch case (params (npos, nbatch, 3), concatenated signal)."""
    off = np.concatenate([[0], np.cumsum(case["siglen"])])
    return [fn(case["params"][:, b], case["signal"][off[b]:off[b + 1]], case["back_prob"], *args)
            for b in range(len(case["siglen"]))]
