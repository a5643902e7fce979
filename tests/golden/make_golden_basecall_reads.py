#!/usr/bin/env python
"""Generate tests/golden/basecall_reads.npz with the GENUINE reference: maths.med_mad and
basecall_helpers.chunk_read on the seeded signals of tests/basecall_support.py, and basecall_helpers.stitch_chunks,
flipflopfings.path_to_str, qscores.path_errprobs_to_qstring on per-chunk paths with realistic dwell (confident scores
through the oracle's Viterbi and errprobs_from_trans).  Run tests/golden/make_golden.py first (it builds the scratch
copy of the reference); only expected OUTPUTS, the tail's small inputs and checksums are stored.

    python tests/golden/make_golden_basecall_reads.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
from tests import basecall_support as bs  # noqa: E402
from tests.golden import make_golden  # noqa: E402


def main():
    make_golden.build_reference()
    import torch
    import oracle
    from taiyaki import basecall_helpers, flipflopfings, maths, qscores
    if not hasattr(np.ndarray, "tostring"):         # numpy 2 dropped the alias the reference uses
        def qchar_from_qscore(score, zerochar=33):
            return (np.array(score) + zerochar + 0.5).astype(np.int8).tobytes().decode("ascii")
        qscores.qchar_from_qscore = qchar_from_qscore
    oracle.build()
    out = {}
    for name in bs.SIGNALS:
        x = bs.signal(name)
        med, mad = maths.med_mad(x)
        assert med.dtype == np.float32 and mad.dtype == np.float32, (med.dtype, mad.dtype)
        out[name + "/med"], out[name + "/mad"] = med, mad
        # bin/basecall.py:77-90 med_mad_norm; a signal whose MAD is 0 has no normalised form: its chunks are raw
        normed = ((x - med) / mad).astype("f4") if mad > 0 else x
        chunks, starts, ends = basecall_helpers.chunk_read(normed, bs.CHUNK, bs.OVERLAP)
        out[name + "/chunk_starts"], out[name + "/chunk_ends"] = np.asarray(starts), np.asarray(ends)
        out[name + "/chunks_shape"] = np.array(chunks.shape)
        out[name + "/chunks_crc"] = np.array(bs.crc(chunks), dtype=np.uint32)
        out[name + "/first_chunk"] = np.ascontiguousarray(chunks[:, 0, 0])
        out[name + "/last_chunk"] = np.ascontiguousarray(chunks[:, -1, 0])
    for name, spec in bs.TAILS.items():
        scores = bs.tail_scores(spec)
        _, trans = oracle.flipflop_logz_grad(scores)
        _, _, path = oracle.flipflop_viterbi(scores)
        err = oracle.errprobs_from_trans(trans, path)
        chunk = spec["T"] * spec["stride"]
        _, starts, ends = basecall_helpers.chunk_read(np.zeros(bs.tail_siglen(spec), dtype="f4"), chunk, spec["overlap"])
        assert len(starts) == spec["N"] and spec["overlap"] > 0
        tpath, terr = torch.tensor(path), torch.tensor(err)
        spath = basecall_helpers.stitch_chunks(tpath, starts, ends, spec["stride"]).numpy()
        serr = basecall_helpers.stitch_chunks(terr, starts, ends, spec["stride"])
        # the reference never meets e <= 0 on these inputs (its own answer there is a float -> int8 overflow)
        picked = serr.numpy()[1:]
        assert picked.min() > 1e-9 and picked.max() < 1.0, (picked.min(), picked.max())
        assert (np.diff(path, axis=0) == 0).mean() > 0.3, "no dwell"
        out["tail/%s/path" % name] = path.astype(np.int8)
        out["tail/%s/errprobs" % name] = err
        out["tail/%s/chunk_starts" % name], out["tail/%s/chunk_ends" % name] = np.asarray(starts), np.asarray(ends)
        out["tail/%s/stitched_path" % name] = spath.astype(np.int8)
        seq = flipflopfings.path_to_str(spath, alphabet="ACGT", include_first_source=False)
        out["tail/%s/seq" % name] = np.frombuffer(seq.encode("ascii"), dtype=np.uint8)
        for tag, (scale, offset) in bs.QSETTINGS.items():
            q = qscores.path_errprobs_to_qstring(serr, spath, scale, offset)
            assert len(q) == len(seq)
            out["tail/%s/%s" % (name, tag)] = np.frombuffer(q.encode("ascii"), dtype=np.uint8)
    path = os.path.join(HERE, "basecall_reads.npz")
    np.savez_compressed(path, **out)
    print("wrote basecall_reads.npz: %d arrays, %d bytes" % (len(out), os.path.getsize(path)))


if __name__ == "__main__":
    main()
