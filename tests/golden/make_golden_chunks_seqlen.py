#!/usr/bin/env python
"""Generate tests/golden/chunks_seqlen.npz with the GENUINE reference (this container only):
signal_mapping.SignalMapping.get_chunk_with_sequence_length, Chunk.apply_filters,
chunk_selection.sample_filter_parameters / sample_chunks(chunk_len_means_sequence_len=True) and the batch of
bin/train_squiggle.py:201-209, on reads from taiyaki_amd.synth.mapped_reads.  The three modules it needs
(taiyaki.signal_mapping, taiyaki.chunk_selection, taiyaki.maths) are numpy only and import from the reference tree
as it stands; the embedding table is the reference's own expression, evaluated from squiggle_match.pyx:18-22 (that
module needs a build, its table does not).  The reference draws (read number, start base) from numpy's global
generator; the draws are recorded by wrapping np.random.randint so that the fixture holds the candidate list next
to the expected outputs.  Only OUTPUTS and draws are stored, numbers all of them.

Every spec is recorded twice, by the filter parameters it is filtered with:
  seq   sample_filter_parameters(..., chunk_len_means_sequence_len=True): from chunks of `bases` bases
  smp   sample_filter_parameters(...) as bin/train_squiggle.py:136-140 calls it: from chunks of `bases` SAMPLES

    python tests/golden/make_golden_chunks_seqlen.py
"""
import os
import re
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests.golden.make_golden import REF  # noqa: E402

REASONS = ("pass", "emptysequence", "emptysignal", "tooshort", "nullmapping", "pathbuffer", "meandwell", "maxdwell")
FORMS = ("seq", "smp")


def _spec(nreads, seed, bases, nsample, nwant, filter_mean_dwell=3.0, filter_max_dwell=10.0, min_pass=0.5):
    return dict(nreads=nreads, seed=seed, bases=bases, nsample=nsample, nwant=nwant,
                filter_mean_dwell=filter_mean_dwell, filter_max_dwell=filter_max_dwell, min_pass=min_pass,
                path_buffer=1.1, stride=1)


# reads are synth.mapped_reads(nreads, seed); the filter defaults are the reference's command line's
SPECS = {
    "r40b60": _spec(40, 171, 60, 60, 32),               # tooshort, maxdwell and meandwell all occur
    "r30b150": _spec(30, 172, 150, 40, 24),             # a short batch
    "r30b300": _spec(30, 173, 300, 40, 16),             # the trainer's chunk: few reads are long enough
    "r30b40tight": _spec(30, 174, 40, 50, 48, filter_mean_dwell=1.0, filter_max_dwell=4.0, min_pass=0.2),
    "r6b100": _spec(6, 176, 100, 12, 64, filter_max_dwell=6.0, min_pass=0.25),     # more chunks than reads
    "r20b1": _spec(20, 177, 1, 30, 20),                 # one base per chunk: no dwell difference
}


def spec_reads(spec):
    from taiyaki_amd import synth
    return synth.mapped_reads(spec["nreads"], spec["seed"])


def reference_embedding_table():
    text = open(os.path.join(REF, "taiyaki", "squiggle_match", "squiggle_match.pyx")).read()
    scope = {"np": np}
    exec(re.search(r"^_cartesian_tetrahedron = np\.array\(.*?dtype=np\.float32\)", text, re.S | re.M).group(), scope)
    return scope["_cartesian_tetrahedron"]


def main():
    sys.path.insert(0, REF)
    from taiyaki import chunk_selection, signal_mapping
    table = reference_embedding_table()
    out = {}
    for name, spec in SPECS.items():
        reads = spec_reads(spec)
        sms = [signal_mapping.SignalMapping(
            r["Ref_to_signal"], r["Reference"], signalstart=0,
            **{k: r[k] for k in ("shift_frompA", "scale_frompA", "range", "offset", "digitisation",
                                 "read_id", "Dacs")}) for r in reads]
        assert all(sm.check() == sm.pass_str for sm in sms)
        ids = [r["read_id"] for r in reads]
        for form in FORMS:
            draws = []
            real_randint = np.random.randint

            def recording_randint(high):
                v = real_randint(high)
                draws.append((int(high), int(v)))
                return v
            np.random.randint = recording_randint
            try:
                np.random.seed(spec["seed"])
                fp = chunk_selection.sample_filter_parameters(
                    sms, spec["nsample"], spec["bases"], spec["filter_mean_dwell"], spec["filter_max_dwell"],
                    spec["min_pass"], spec["stride"], spec["path_buffer"],
                    chunk_len_means_sequence_len=(form == "seq"))
                ndraw_fp = len(draws)
                chunks, rej = chunk_selection.sample_chunks(
                    sms, spec["nwant"], spec["bases"], fp, chunk_len_means_sequence_len=True)
            finally:
                np.random.randint = real_randint
            key = "%s/%s/" % (name, form)
            out[key + "median_mad"] = np.array([fp.median_meandwell, fp.mad_meandwell])
            out[key + "draws_filter"] = np.array(draws[:ndraw_fp], dtype=np.int64).reshape(-1, 2)
            out[key + "draws_batch"] = np.array(draws[ndraw_fp:], dtype=np.int64).reshape(-1, 2)
            out[key + "rejections"] = np.array([rej.get(k, 0) for k in REASONS], dtype=np.int64)
            siglens = [c.sig_len for c in chunks]
            print(name, form, "accepted", len(chunks), "of", spec["nwant"], dict(rej), "median/mad",
                  fp.median_meandwell, fp.mad_meandwell, "siglen", (min(siglens), max(siglens)) if chunks else None)
            out[key + "chunk_read"] = np.array([ids.index(c.read_id) for c in chunks], dtype=np.int64)
            out[key + "chunk_start"] = np.array([c.start_sample for c in chunks], dtype=np.int64)
            out[key + "chunk_maxdwell"] = np.array([c.max_dwell for c in chunks], dtype=np.int64)
            out[key + "chunk_siglen"] = np.array(siglens, dtype=np.int64)
            # the batch of bin/train_squiggle.py:201-209, both directions
            for tag, revop in (("fwd", np.array), ("rev", np.flip)):
                seqs = [revop(c.sequence) for c in chunks]
                embed = [table[s] for s in seqs]                # embed_sequence(..., alphabet=None), :116-120
                cur = [revop(c.current) for c in chunks]
                out[key + "seqs_" + tag] = (np.stack(seqs, axis=1) if chunks
                                            else np.zeros((spec["bases"], 0))).astype(np.int8)
                out[key + "embed_" + tag] = (np.stack(embed, axis=1) if chunks
                                             else np.zeros((spec["bases"], 0, 3))).astype(np.float32)
                out[key + "signal_" + tag] = (np.concatenate(cur) if chunks else np.zeros(0)).astype(np.float32)
    path = os.path.join(HERE, "chunks_seqlen.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
