#!/usr/bin/env python
"""The genuine reference C's answers on the cases the CPU pinning tests hold it to, stored so that the
tests stand without it (refc_answers.npz).  oracle/Makefile compiles the reference sources into
oracle/_ref/ only where they lie on disk; everywhere else tests/test_oracle_pinning.py and
tests/test_beamsearch.py compare the restatement with these stored answers, and where oracle/_ref
exists they compare with the live library as well.

The case lists live here and the tests import them, so both walk the same inputs in the same order.

    make -C oracle && python tests/golden/make_golden_refc.py
"""
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from taiyaki_amd import synth  # noqa: E402

PATH = os.path.join(HERE, "refc_answers.npz")
NMODS = (1, 1, 0, 0)        # = tests/golden/cases.py

# tests/test_oracle_pinning.py::test_restatement_equals_reference_c: (T, N, seed)
RESTATEMENT_CASES = [(60, 5, 3), (257, 9, 4)]
RESTATEMENT_SHARPEN = 1.3
# ...::test_float64_witness_agrees_with_the_fp32_restatement_and_the_reference: (T, seqlens, mods, sharpen)
WITNESS_CASES = ((7, [6, 2], None, 1.0), (50, [25, 40, 7, 12], None, 2.5), (50, [30, 17, 0], None, 1.0),
                 (60, [25, 40, 7], (1, 1, 0, 0), 1.0), (60, [25, 40, 7], (1, 1, 0, 0), 2.5),
                 (200, [90, 150, 30, 180], None, 1.0))
# ...::test_empty_read_inside_a_batch_is_scored_apart
EMPTY_T, EMPTY_SEQLENS, EMPTY_SEED = 40, (12, 0, 20, 9, 0), 5


def restatement_input(T, N, seed, mods=None):
    return synth.crf_case(T, N, seed, nmods_per_base=mods)


def witness_input(T, seqlens, mods):
    return synth.crf_case(T, len(seqlens), 91 + T, seqlens=np.array(seqlens, dtype=np.int32), nmods_per_base=mods)


def empty_read_input():
    seqlens = np.array(EMPTY_SEQLENS, dtype=np.int32)
    return synth.crf_case(EMPTY_T, len(seqlens), EMPTY_SEED, seqlens=seqlens), seqlens


def empty_read_raw_call(oracle_mod, inp, seqlens):
    """The raw reference call on the batch with an empty read inside (ctc.pyx:127-129's move layout)."""
    nbase = 4
    off = np.concatenate([[0], np.cumsum(seqlens)])
    move = np.concatenate([oracle_mod.flipflop_indices(inp["seqs"][off[n]:off[n + 1]], seqlens[n:n + 1], nbase)[0]
                           [:max(seqlens[n] - 1, 0)] for n in range(len(seqlens))] + [np.zeros(2, dtype=np.uintp)])
    stay = oracle_mod.flipflop_indices(inp["seqs"], seqlens, nbase)[1]
    return oracle_mod._seq_call(oracle_mod.ref(), "", inp["scores"], move, stay, seqlens)


def beam_random_cases():
    """tests/test_beamsearch.py::test_restatement_matches_the_reference_library_on_random_cases:
    (scores, beam_cut, beam_width, guided) for 10 continuous and 6 tie-heavy cases."""
    from tests.test_beamsearch import quantised_scores
    rng = np.random.RandomState(4)
    out = []
    for k in range(10):
        T = int(rng.randint(5, 160))
        sc = (synth.scores(T, 1, 40, 900 + k)[:, 0, :] * np.float32(rng.uniform(0.3, 1.6))).astype(np.float32)
        w, cut, g = int(rng.randint(1, 13)), float(rng.choice([0.0, 0.0, 0.01, 0.2])), bool(rng.randint(2))
        out.append((sc, cut, w, g))
    for k in range(6):
        w, cut, g = int(rng.choice([3, 5, 12])), float(rng.choice([0.0, 0.05])), bool(rng.randint(2))
        out.append((quantised_scores(int(rng.randint(20, 140)), 50 + k), cut, w, g))
    return out


def lattice_cases():
    """tests/test_beamsearch.py::test_lattice_restatement_against_reference_library_and_unit_test: (scores, init)."""
    rng = np.random.RandomState(8)
    out = []
    for k in range(6):
        sc = (rng.randn(int(rng.randint(1, 90)), 40) * 2).astype(np.float32)
        init = None if k % 2 else (rng.randn(8) * 3).astype(np.float32)
        out.append((sc, init))
    return out


def harness_summary(exe):
    """The lines of a reference harness's output that are not per-element derivative dumps."""
    out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    return [ln for ln in out.splitlines() if ln and not ln[0].isspace() and not ln.endswith(":")]


def main():
    import oracle
    from oracle import beam
    assert oracle.ref_available() and beam.ref_available(), "build oracle/_ref first (make -C oracle)"
    out = {}
    ref_dir = os.path.join(ROOT, "oracle", "_ref")
    out["harness/crf_twostate_test"] = np.array(harness_summary(os.path.join(ref_dir, "crf_twostate_test")))
    out["harness/cat_mod_test"] = np.array(harness_summary(os.path.join(ref_dir, "cat_mod_test")))
    for T, N, seed in RESTATEMENT_CASES:
        key = "restatement/%d_%d_%d/" % (T, N, seed)
        inp = restatement_input(T, N, seed)
        out[key + "crf_loss"], out[key + "crf_grad"] = oracle.crf_flipflop_loss(
            inp["scores"], inp["seqs"], inp["seqlens"], RESTATEMENT_SHARPEN, use_ref=True)
        inp = restatement_input(T, N, seed, NMODS)
        out[key + "catmod_loss"], out[key + "catmod_grad"] = oracle.cat_mod_flipflop_loss(
            inp["scores"], inp["seqs"], inp["seqlens"], inp["mod_cats"], inp["can_mods_offsets"],
            inp["mod_cat_weights"], 1.0, use_ref=True)
    for i, (T, seqlens, mods, sharp) in enumerate(WITNESS_CASES):
        inp = witness_input(T, seqlens, mods)
        if mods:
            loss, grad = oracle.cat_mod_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], inp["mod_cats"],
                                                      inp["can_mods_offsets"], inp["mod_cat_weights"], sharp, use_ref=True)
        else:
            loss, grad = oracle.crf_flipflop_loss(inp["scores"], inp["seqs"], inp["seqlens"], sharp, use_ref=True)
        out["witness/%d/loss" % i], out["witness/%d/grad" % i] = loss, grad
    inp, seqlens = empty_read_input()
    out["empty/loss"], out["empty/grad"] = oracle.crf_flipflop_loss(inp["scores"], inp["seqs"], seqlens, 1.0, use_ref=True)
    out["empty/raw_loss"] = empty_read_raw_call(oracle, inp, seqlens)[0]
    for k, (sc, cut, w, g) in enumerate(beam_random_cases()):
        seq, score, bwd = beam.ref_beamsearch(sc, cut, w, g)
        out["beam/%d/seq" % k], out["beam/%d/score" % k] = seq, np.float32(score)
        if g:
            out["beam/%d/bwd" % k] = bwd
    for k, (sc, init) in enumerate(lattice_cases()):
        for fwdp in (True, False):
            mat, tot = beam.ref_lattice(sc, init, fwdp)
            key = "lattice/%d/%s/" % (k, "fwd" if fwdp else "bwd")
            out[key + "mat"], out[key + "tot"] = mat, np.float32(tot)
    np.savez_compressed(PATH, **out)
    print("%s: %d arrays, %d bytes" % (PATH, len(out), os.path.getsize(PATH)))


if __name__ == "__main__":
    main()
