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


# ----------------------------------------------------------------------------------------------------------
# Second table (tests/test_squiggle_instantiations.py, tests/golden/squiggle_lanes.npz): every positions-per-
# lane instantiation R of csrc/squiggle_kernels.hip at three kinds of npos -- "first", the smallest npos that
# selects the R; "full", npos = 64 R (no idle lane, the last position is the last of its lane); "mid", the last
# position in the middle of a lane with idle lanes behind it -- plus one clipped case per R and the long read
# of test_squiggle_match.py.  The fixture holds the reference's answers only; the inputs come from here.
#
# A case is a batch of reads of different lengths, dwell 2 to 4 samples per position: one sampled from the
# model, a copy of it cut beside a multiple of 64 samples (unless it ends there already), one of the least
# reachable length npos - 1 and one too short to reach the end (its length rotates through SHORT_LENGTHS).
# A clipped case has reads drawn from an inner range of positions between junk samples, and localpen /
# minscore such that the best path enters late and leaves early.
# ----------------------------------------------------------------------------------------------------------
LANE_RULE = [(64, 1), (128, 2), (256, 4), (320, 5), (512, 8), (768, 12), (1024, 16)]       # npos <= .. -> R
SHORT_LENGTHS = (1, 2, 3, 33, 65)
CLIP_LOCALPEN, CLIP_MINSCORE, CLIP_JUNK = 0.5, 8.0, 25
LONG = "long1024"               # random_batch(1024, 1, 5): 8409 samples in one read

_FIRST = [65, 129, 257, 321, 513, 769]                  # (npos 1 is in CASES)
_FULL = [64, 128, 256, 320, 512, 768, 1024]
# (R 1 and 2 have no middle of a lane; 199 and CASES' 299 are the last of theirs, 201 and 302 are not)
_MID = [100, 200, 202, 303, 450, 700, 1000]
_CLIP = [40, 100, 200, 300, 450, 700, 1000]


def lanes_r(npos):
    """Positions per lane of the kernels' dispatch rule (0: beyond the build)."""
    return next((r for lim, r in LANE_RULE if npos <= lim), 0)


def _lane_table():
    table, k = {}, 0
    for kind, values in (("first", _FIRST), ("full", _FULL), ("mid", _MID), ("clip", _CLIP)):
        for npos in values:
            short = 0 if kind == "clip" else SHORT_LENGTHS[k % 5]
            while short >= npos - 1:                    # (65 samples reach the end of 64 or 65 positions)
                short = SHORT_LENGTHS[(SHORT_LENGTHS.index(short) + 1) % 5]
            table["%s%d" % (kind, npos)] = (npos, kind, 0.3 if k % 2 else 1e-15, short, 100 + k)
            k += 1
    return table


# name -> (npos, kind, back_prob, length of the unreachable read (clipped cases have none), seed)
LANE_CASES = _lane_table()
LANE_NAMES = list(LANE_CASES) + [LONG]


def lane_params(npos, rng):
    p = read_params(npos, rng)
    dwell = rng.uniform(2.0, 4.0, npos)
    p[:, 2] = np.log(1.0 / (dwell - 1.0))
    return p


def sample_range(p, rng, back_prob, lo, hi):
    """`sample_signal` over the positions lo .. hi only: starts in lo, ends with the move out of hi."""
    out, pos = [], lo
    while True:
        out.append(p[pos, 0] + rng.laplace(0.0, np.exp(p[pos, 1])))
        mp = (1.0 - back_prob) / (1.0 + np.exp(-p[pos, 2]))
        u = rng.uniform()
        if u < mp:
            if pos == hi:
                return np.array(out, dtype=np.float32)
            pos += 1
        elif u < mp + back_prob and pos > lo:
            pos -= 1


def _emit(p, positions, rng):
    return (p[positions, 0] + rng.laplace(0.0, np.exp(p[positions, 1]))).astype(np.float32)


def make_lane_case(name):
    if name == LONG:
        return random_batch(1024, 1, 5)
    npos, kind, back_prob, short, seed = LANE_CASES[name]
    rng = np.random.RandomState(seed)
    back = 0.01 if back_prob > 0.1 else 0.0
    localpen = minscore = None
    if kind == "clip":
        localpen, minscore = CLIP_LOCALPEN, CLIP_MINSCORE
        params = [lane_params(npos, rng) for _ in range(2)]
        sigs = []
        for b, (lo, hi) in enumerate([(npos // 16 + 2, npos - npos // 14 - 2), (npos // 5, npos - npos // 3)]):
            junk = [rng.uniform(-6.0, 6.0, CLIP_JUNK + 7 * b).astype(np.float32) for _ in range(2)]
            sigs.append(np.concatenate([junk[0], sample_range(params[b], rng, back, lo, hi), junk[1]]))
    else:
        params = [lane_params(npos, rng) for _ in range(4)]
        full = sample_range(params[0], rng, back, 0, npos - 1)
        sigs = [full]
        cut = (len(full) - 1) // 64 * 64 + 1            # the largest 64 k + 1 <= len(full)
        if len(full) % 64 > 1 and cut >= npos - 1:
            params[1] = params[0]
            sigs.append(full[:cut].copy())
        else:
            del params[1]
        sigs.append(_emit(params[-2], np.arange(1, npos), rng))             # one move per sample
        sigs.append(sample_range(params[-1], rng, back, 0, npos - 1)[:short])
        assert len(sigs[-1]) == short < npos - 1
    return dict(params=np.ascontiguousarray(np.stack(params, axis=1)), signal=np.concatenate(sigs),
                siglen=np.array([len(s) for s in sigs], dtype=np.int32), back_prob=back_prob,
                localpen=localpen, minscore=minscore)


def digest(case):
    """What the fixture keeps of a case's inputs: the lengths and the float64 sums of params and signal."""
    return case["siglen"].astype(np.int32), np.array([case["params"].sum(dtype=np.float64),
                                                      case["signal"].sum(dtype=np.float64)])
