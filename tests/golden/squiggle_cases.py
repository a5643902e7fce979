"""Inputs of the squiggle-match tests (tests/test_squiggle_match.py) and of the fixture writer
(tests/golden/make_golden_squiggle.py): synthetic reads sampled from the model itself, so that
alignments have clear margins.  Per position a level ~ N(0, 1), a log-scale in [-1.6, -1.0] and a
move logit; dwell times are geometric in the move probability and the noise is Laplace.

A case is a dict: params (npos, nbatch, 3) float32, signal float32, siglen (nbatch) int32, back_prob,
localpen and minscore (None = the reference's LARGE_LOG_VAL).
"""
import numpy as np

# name -> (npos, nbatch, back_prob, localpen, minscore, seed)
CASES = {
    "ragged5": (5, 3, 1e-15, None, None, 11),
    "npos1": (1, 2, 1e-15, None, None, 12),
    "npos37_back03": (37, 4, 0.3, None, None, 13),
    "npos37_local": (37, 3, 1e-15, 40.0, 6.0, 14),
    "npos300": (300, 2, 1e-15, None, None, 15),
    "npos300_back03_local": (300, 1, 0.3, 60.0, 8.0, 16),
    "unreachable": (37, 3, 1e-15, None, None, 17),
}
# the reference's own harness (c_squiggle_match.c SQUIGGLE_TEST): its arrays are read from the fixture
HARNESS = "harness"


def read_params(npos, rng):
    level = rng.normal(0.0, 1.0, npos)
    logsc = rng.uniform(-1.6, -1.0, npos)
    dwell = rng.uniform(6.0, 10.0, npos)                # mean samples per position
    logit = np.log(1.0 / (dwell - 1.0))                 # plogistic(logit) = 1 / dwell
    return np.stack([level, logsc, logit], axis=1).astype(np.float32)


def sample_signal(p, rng, back_prob=0.0):
    """Samples of one read drawn from its own squiggle: geometric dwell per position (a back step
    with probability back_prob per sample), Laplace noise."""
    npos = p.shape[0]
    out = []
    pos = 0
    while True:
        sc = np.exp(p[pos, 1])
        out.append(p[pos, 0] + rng.laplace(0.0, sc))
        mp = (1.0 - back_prob) / (1.0 + np.exp(-p[pos, 2]))
        u = rng.uniform()
        if u < mp:
            if pos == npos - 1:
                break
            pos += 1
        elif u < mp + back_prob and pos > 0:
            pos -= 1
    return np.array(out, dtype=np.float32)


def make_case(name):
    npos, nbatch, back_prob, localpen, minscore, seed = CASES[name]
    rng = np.random.RandomState(seed)
    params = np.stack([read_params(npos, rng) for _ in range(nbatch)], axis=1)
    sigs = [sample_signal(params[:, b], rng, 0.01 if back_prob > 0.1 else 0.0) for b in range(nbatch)]
    if name == "unreachable":
        sigs[1] = sigs[1][:npos // 3]                   # siglen < npos - 1: the end is out of reach
    return dict(params=np.ascontiguousarray(params), signal=np.concatenate(sigs),
                siglen=np.array([len(s) for s in sigs], dtype=np.int32), back_prob=back_prob,
                localpen=localpen, minscore=minscore)


def random_batch(npos, nbatch, seed, back_prob=1e-15):
    """Seeded batch for the comparisons with the float64 restatement (no fixture)."""
    rng = np.random.RandomState(seed)
    params = np.stack([read_params(npos, rng) for _ in range(nbatch)], axis=1)
    sigs = [sample_signal(params[:, b], rng) for b in range(nbatch)]
    return dict(params=np.ascontiguousarray(params), signal=np.concatenate(sigs),
                siglen=np.array([len(s) for s in sigs], dtype=np.int32), back_prob=back_prob,
                localpen=None, minscore=None)


def from_fixture(gold, name):
    """A case as the fixture stores it (NaN localpen / minscore = None)."""
    lp, ms = float(gold[name + "/localpen"]), float(gold[name + "/minscore"])
    return dict(params=gold[name + "/params"], signal=gold[name + "/signal"], siglen=gold[name + "/siglen"],
                back_prob=float(gold[name + "/back_prob"]), localpen=None if np.isnan(lp) else lp,
                minscore=None if np.isnan(ms) else ms)


NAMES = list(CASES) + [HARNESS]
EMBED_SEQUENCE = "ACGTTGCAAGTC"
