#!/usr/bin/env python
"""Writes tests/golden/squiggle_small.npz: the reference squiggle match's answers on the cases of
tests/golden/squiggle_cases.py, so that tests/test_squiggle_match.py stands without the reference; and
tests/golden/squiggle_lanes.npz: its answers alone (cost, grad, vcost, path and a digest of the inputs, which
squiggle_cases.make_lane_case regenerates from their seeds) on the second table there, for
tests/test_squiggle_instantiations.py.

The reference C (taiyaki/squiggle_match/c_squiggle_match.c) is compiled with its own flags
(setup.py: -O3 -fopenmp -std=c99) into a temporary directory outside the tree and called through
ctypes; nothing compiled is kept.  The arrays of the reference's SQUIGGLE_TEST harness are read from
that source file and stored as data.

    python tests/golden/make_golden_squiggle.py /path/to/taiyaki [small] [lanes]        (default: both)
"""
import ctypes
import os
import re
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from tests.golden import squiggle_cases  # noqa: E402

PATH = os.path.join(HERE, "squiggle_small.npz")
LANES_PATH = os.path.join(HERE, "squiggle_lanes.npz")
MAX_BYTES = 1 << 20             # the limit for a committed file
LARGE_LOG_VAL = 50000.0


def _compile(src, tmp):
    lib = os.path.join(tmp, "libsquiggle_ref.so")
    subprocess.run(["cc", "-O3", "-fopenmp", "-std=c99", "-shared", "-fPIC", "-o", lib, src, "-lm"], check=True)
    so = ctypes.CDLL(lib)
    vp, sz, f = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_float
    so.squiggle_match_cost.argtypes = [vp, vp, sz, vp, sz, f, vp]
    so.squiggle_match_grad.argtypes = [vp, vp, sz, vp, sz, f, vp]
    so.squiggle_match_viterbi_path.argtypes = [vp, vp, sz, vp, sz, f, f, f, vp, vp]
    return so


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def run_reference(so, case):
    """(cost, grad, viterbi cost, path) as squiggle_match.pyx returns them (negated)."""
    params = np.ascontiguousarray(case["params"], dtype=np.float32)
    signal = np.ascontiguousarray(case["signal"], dtype=np.float32)
    siglen = np.ascontiguousarray(case["siglen"], dtype=np.int32)
    npos, nbatch = params.shape[:2]
    pb = case["back_prob"]
    lp = LARGE_LOG_VAL if case["localpen"] is None else case["localpen"]
    ms = LARGE_LOG_VAL if case["minscore"] is None else case["minscore"]
    cost = np.zeros(nbatch, dtype=np.float32)
    so.squiggle_match_cost(_p(signal), _p(siglen), nbatch, _p(params), npos, pb, _p(cost))
    grad = np.zeros_like(params)
    so.squiggle_match_grad(_p(signal), _p(siglen), nbatch, _p(params), npos, pb, _p(grad))
    vcost = np.zeros(nbatch, dtype=np.float32)
    path = np.zeros(signal.shape, dtype=np.int32)
    so.squiggle_match_viterbi_path(_p(signal), _p(siglen), nbatch, _p(params), npos, pb, lp, ms, _p(path), _p(vcost))
    return -cost, -grad, -vcost, path


def _floats(text, name):
    body = re.search(r"\b%s\[[^\]]*\]\s*=\s*\{(.*?)\};" % name, text, flags=re.S).group(1)
    body = re.sub(r"//[^\n]*", "", body)
    return [float(v.rstrip("f")) for v in re.findall(r"[-+]?\d+\.?\d*(?:[eE][-+]?\d+)?f?", body)]


def harness_case(src):
    text = open(src).read()
    text = text[text.index("#ifdef SQUIGGLE_TEST"):]
    signal = np.array(_floats(text, "test_signal"), dtype=np.float32)
    siglen = np.array(_floats(text, "test_siglen"), dtype=np.int32)
    npos = int(re.search(r"const size_t npos = (\d+);", text).group(1))
    nbatch = int(re.search(r"const size_t nbatch = (\d+);", text).group(1))
    params = np.array(_floats(text, "test_param"), dtype=np.float32).reshape(npos, nbatch, 3)

    def const(name):
        return float(re.search(r"const float %s = ([-+0-9.eE]+)f?;" % name, text).group(1))
    return dict(params=params, signal=signal, siglen=siglen, back_prob=const("prob_back"),
                localpen=const("localpen"), minscore=const("minscore"))


def embed_expected(seq):
    """The tetrahedron embedding (squiggle_match.pyx:18-22, 114-123), restated."""
    verts = np.array([[1.0, 0.0, -1.0 / np.sqrt(2.0)], [-1.0, 0.0, -1.0 / np.sqrt(2.0)],
                      [0.0, 1.0, 1.0 / np.sqrt(2.0)], [0.0, -1.0, 1.0 / np.sqrt(2.0)]], dtype=np.float32)
    return verts[["ACGT".index(b) for b in seq]]


def write_lanes(src):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = _compile(src, tmp)
        for name in squiggle_cases.LANE_NAMES:
            case = squiggle_cases.make_lane_case(name)
            cost, grad, vcost, path = run_reference(so, case)
            out[name + "/siglen"], out[name + "/sums"] = squiggle_cases.digest(case)
            out[name + "/cost"], out[name + "/grad"] = cost, grad
            out[name + "/vcost"], out[name + "/path"] = vcost, path
            print("%-10s npos %4d siglen %s cost %s" % (name, case["params"].shape[0], case["siglen"], cost))
    np.savez_compressed(LANES_PATH, **out)
    size = os.path.getsize(LANES_PATH)
    print("wrote %s (%d bytes)" % (LANES_PATH, size))
    assert size < MAX_BYTES, "the fixture must stay under 1 MiB"


def main(reference_root, which=("small", "lanes")):
    src = os.path.join(reference_root, "taiyaki", "squiggle_match", "c_squiggle_match.c")
    if "lanes" in which:
        write_lanes(src)
    if "small" not in which:
        return
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        so = _compile(src, tmp)
        cases = {name: squiggle_cases.make_case(name) for name in squiggle_cases.CASES}
        cases[squiggle_cases.HARNESS] = harness_case(src)
        for name, case in cases.items():
            cost, grad, vcost, path = run_reference(so, case)
            for k in ("params", "signal", "siglen"):
                out[name + "/" + k] = case[k]
            out[name + "/back_prob"] = np.float32(case["back_prob"])
            for k in ("localpen", "minscore"):
                out[name + "/" + k] = np.float32(np.nan if case[k] is None else case[k])
            out[name + "/cost"], out[name + "/grad"] = cost, grad
            out[name + "/vcost"], out[name + "/path"] = vcost, path
            print("%-22s npos %4d nbatch %d siglen %s cost %s" % (name, case["params"].shape[0],
                                                                  case["params"].shape[1], case["siglen"], cost))
    out["embed/sequence"] = np.array(squiggle_cases.EMBED_SEQUENCE)
    out["embed/expected"] = embed_expected(squiggle_cases.EMBED_SEQUENCE)
    np.savez_compressed(PATH, **out)
    print("wrote %s (%d bytes)" % (PATH, os.path.getsize(PATH)))


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else os.environ.get("TAIYAKI_REFERENCE", "../taiyaki"),
         tuple(sys.argv[2:]) or ("small", "lanes"))
