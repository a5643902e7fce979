#!/usr/bin/env python
"""flipflop_remap benchmark.

    python tools/remapbench.py [--blocks 20000] [--bases 9000] [--reads 256]
    python tools/remapbench.py --pipeline [--pipeline-reads 1 8 64]

--pipeline times `prepare_mapping_funcs.remap_batch` against the per-read chain (the same model at N = 1 per read, then
the existing batch remap and Ref_to_signal) on reads of 20 000 - 100 000 samples, for the size-96 mGru (stride 4) and a
size-256 mLstm: after a warm-up of both, the two sides take five turns each; a call ends in its download.

One read alone (latency of the serial time loop + traceback) and a batch of reads in one launch
(one workgroup per read).  The host-path comparison (numpy restatement of the reference: the
same ~12 numpy calls per time step as taiyaki/flipflop_remap.py) lives with the test
infrastructure: `python -m tests.helpers.cpu_legs remap`.
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import flipflop_remap as fr, synth  # noqa: E402


def pipeline(read_counts):
    from taiyaki_amd import models, prepare_mapping_funcs as pm
    dev = torch.device("cuda:0")
    rs = np.random.RandomState(17)
    nets = [("mGru 96 stride 4", models.mGru_flipflop(size=96, stride=4)), ("mLstm 256 stride 5", models.mLstm_flipflop(size=256, stride=5))]
    for name, net in nets:
        torch.manual_seed(3)
        net = synth.excite_network(net).to(dev).eval()
        stride = pm.model_stride(net)
        for nread in read_counts:
            lens = np.linspace(20000, 100000, nread).astype(int) if nread > 1 else np.array([60000])
            sigs = [(90 + 12 * rs.standard_normal(n)).astype(np.float32) for n in lens]
            refs = ["".join(rs.choice(list("ACGT"), size=int(0.4 * n / stride))) for n in lens]
            params = [dict(trim_start=0, trim_end=0, shift=90.0, scale=12.0)] * nread

            def batch():
                with torch.no_grad():
                    return pm.remap_batch(sigs, refs, net, params)

            def per_read():
                with torch.no_grad():
                    scores = [net(((torch.from_numpy(s).to(dev) - 90.0) / 12.0)[:, None, None])[:, 0] for s in sigs]
                    score, paths = fr.flipflop_remap_batch(scores, refs, localpen=0.0)
                    return score, paths, fr.ref_to_signal_from_remapping_paths(paths, [len(r) for r in refs], stride, 0,
                                                                                [len(s) for s in sigs], device=dev)
            batch(), per_read()
            tb, tp = [], []
            for _ in range(5):
                for fn, out in ((batch, tb), (per_read, tp)):
                    torch.cuda.synchronize()
                    t0 = time.time()
                    fn()
                    out.append((time.time() - t0) * 1e3)
            print("%s, %d reads (%d - %d samples): remap_batch %s ms; per read %s ms; medians %.1f / %.1f"
                  % (name, nread, lens.min(), lens.max(), " ".join("%.1f" % t for t in tb), " ".join("%.1f" % t for t in tp),
                     np.median(tb), np.median(tp)), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=20000)
    ap.add_argument("--bases", type=int, default=9000)
    ap.add_argument("--reads", type=int, default=256)
    ap.add_argument("--cpu-reads", type=int, default=0, help="(kept for old command lines; no effect)")
    ap.add_argument("--pipeline", action="store_true", help="time remap_batch against the per-read chain")
    ap.add_argument("--pipeline-reads", type=int, nargs="*", default=[1, 8, 64])
    args = ap.parse_args()
    if args.pipeline:
        return pipeline(args.pipeline_reads)
    dev = torch.device("cuda:0")
    T, M = args.blocks, args.bases
    sc = torch.tensor(synth.scores(T, 1, 40, 5)[:, 0, :], device=dev)
    bases = synth.randint(5, 21, M, 4)
    step, stay = fr.remap_indices(bases)
    fr.map_to_crf_viterbi(sc, step, stay, 3.0)
    torch.cuda.synchronize()
    t0 = time.time()
    reps = 5
    for _ in range(reps):
        score, path = fr.map_to_crf_viterbi(sc, step, stay, 3.0)
    one = (time.time() - t0) / reps
    print("one read   T=%d M=%d: %8.2f ms (incl. index upload, path download)  score %.3f" % (T, M, one * 1e3, score))
    n = args.reads
    scs = [sc] * n
    fr.map_to_crf_viterbi_batch(scs[:2], [step] * 2, [stay] * 2, 3.0)
    torch.cuda.synchronize()
    bts = []
    for _ in range(3):                  # (the first full-size call also pays for its workspaces)
        torch.cuda.synchronize()
        t0 = time.time()
        s, p = fr.map_to_crf_viterbi_batch(scs, [step] * n, [stay] * n, 3.0)
        bts.append(time.time() - t0)
    print("batch of %d, call by call: %s ms" % (n, ", ".join("%.1f" % (b * 1e3) for b in bts)))
    bt = min(bts)
    assert np.all(s == score) and all(np.array_equal(x, path) for x in p[:4])
    print("batch of %d: %8.2f ms = %.2f ms per read = %.0f reads/s (%.1f M blocks/s)"
          % (n, bt * 1e3, bt / n * 1e3, n / bt, n * T / bt / 1e6))


if __name__ == "__main__":
    main()
