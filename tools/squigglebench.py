#!/usr/bin/env python
"""Times the squiggle match on the GPU at bin/train_squiggle.py's default shape: 100 reads x 300
positions x 2400-3000 samples (fixed seed).  Cost, gradient (forward + backward sweep), Viterbi path
and squiggle_match_loss forward + backward, each timed with device events after warm-up; prints one
JSON line (milliseconds per call, median and min over --steps).

    python tools/squigglebench.py [--steps 20] [--warmup 3] [--nbatch 100] [--npos 300]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, squiggle_match as sm  # noqa: E402


def batch(nbatch, npos, lo, hi, seed):
    rng = np.random.RandomState(seed)
    params = np.stack([rng.normal(0, 1, (nbatch, npos)), rng.uniform(-1.6, -1.0, (nbatch, npos)),
                       rng.normal(-2.0, 0.3, (nbatch, npos))], axis=2).transpose(1, 0, 2)
    params = np.ascontiguousarray(params, dtype=np.float32)
    siglen = rng.randint(lo, hi + 1, nbatch).astype(np.int32)
    sigs = []
    for b in range(nbatch):
        pos = (np.arange(siglen[b]) * npos) // siglen[b]
        sigs.append(params[pos, b, 0] + rng.laplace(0, np.exp(params[pos, b, 1])))
    return params, np.concatenate(sigs).astype(np.float32), siglen


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--nbatch", type=int, default=100)
    ap.add_argument("--npos", type=int, default=300)
    ap.add_argument("--back-prob", type=float, default=1e-15)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("squigglebench needs a GPU (the squiggle match has no CPU fallback)")
    dev = torch.device("cuda:0")
    params, signal, siglen = batch(a.nbatch, a.npos, 2400, 3000, 7)
    p = torch.from_numpy(params).to(dev)
    s = torch.from_numpy(signal).to(dev)
    n = torch.from_numpy(siglen.astype(np.int64)).to(dev)
    _lib.set_strict(False)

    def loss_step():
        q = p.clone().requires_grad_()
        sm.squiggle_match_loss(q, s, n, a.back_prob).sum().backward()

    ops = {"cost": lambda: sm.cost_dev(p, s, n, a.back_prob),
           "grad": lambda: sm.grad_dev(p, s, n, a.back_prob),
           "path": lambda: sm.path_dev(p, s, n, a.back_prob),
           "loss_fwd_bwd": loss_step}
    out = {"nbatch": a.nbatch, "npos": a.npos, "samples": int(siglen.sum()), "back_prob": a.back_prob,
           "device": torch.cuda.get_device_name(dev)}
    for name, fn in ops.items():
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        times = []
        for _ in range(a.steps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            times.append(e0.elapsed_time(e1))
        out[name + "_ms"] = round(float(np.median(times)), 3)
        out[name + "_min_ms"] = round(float(np.min(times)), 3)
    _lib.raise_if_nonfinite()
    out["us_per_sample_step_cost"] = round(1e3 * out["cost_ms"] / float(siglen.max()), 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
