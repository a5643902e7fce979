#!/usr/bin/env python
"""Times the squiggle predictor network (models.squiggle_predictor) on the GPU: the fused operator
(csrc/squiggle_net.hip) against the per-layer path (layers.USE_HIP_SQUIGGLE_NET = False), the switch on and off in
turns inside one process, --turns turns a side, per turn the median of --calls calls timed with device events after
warm-up.  One JSON line per turn and, per measurement, one line that says whether EVERY turn of the operator was below
EVERY turn of the per-layer path, with the difference of the medians against the larger of the two sides' max - min
ranges.

  (P 300, N 100, size 32, depth 4, winlen 9): forward alone (no_grad), forward + backward, and the whole trainer step
      with the match loss (train_squiggle.py:216-223 on synthetic signals)
  (P 1000, N 1) and (P 1000, N 64): forward alone, as `predict_squiggle` calls it
  (P 300, N 100, size 64, depth 4, winlen 9): forward alone, forward + backward; and size 64 at (1000, 1), (300, 10),
      (300, 30), (300, 60), with the rule of layers.SquigglePredictor lifted, to see where that rule has to draw its line

    python tools/squigglenetbench.py [--turns 3] [--calls 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import layers, models, squiggle_match, synth  # noqa: E402


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return 1e3 * float(np.median(times))


def compare(tag, fn, a):
    res = {True: [], False: []}
    for turn in range(a.turns):
        for hip in (True, False):
            layers.USE_HIP_SQUIGGLE_NET = hip
            us = timed(fn, a.calls, a.warmup)
            res[hip].append(us)
            print(json.dumps(dict(tag, turn=turn, path="operator" if hip else "per layer", us=round(us, 1))), flush=True)
    layers.USE_HIP_SQUIGGLE_NET = True
    op, ref = res[True], res[False]
    spread = max(max(op) - min(op), max(ref) - min(ref))
    diff = float(np.median(ref) - np.median(op))
    print(json.dumps(dict(tag, operator_us=round(float(np.median(op)), 1), per_layer_us=round(float(np.median(ref)), 1),
                          difference_us=round(diff, 1), larger_range_us=round(spread, 1),
                          difference_over_range=round(diff / spread, 1) if spread > 0 else None,
                          every_operator_turn_below_every_per_layer_turn=max(op) < min(ref))), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("squigglenetbench needs a GPU")
    dev = torch.device("cuda:0")
    torch.backends.cuda.preferred_blas_library("cublas")        # rocBLAS, as bench.py runs the GEMM path
    shapes = [(300, 100, 32, ("fwd", "fwd+bwd", "step")), (1000, 1, 32, ("fwd",)), (1000, 64, 32, ("fwd",)),
              (300, 100, 64, ("fwd", "fwd+bwd"))]
    # size 64 below that: where the rule of layers.SquigglePredictor (SQUIGGLE_NET_64_MAX_ROWS) draws its line
    shapes += [(P, N, 64, ("fwd", "fwd+bwd")) for P, N in ((1000, 1), (300, 10), (300, 30), (300, 60))]
    rule, layers.SQUIGGLE_NET_64_MAX_ROWS = layers.SQUIGGLE_NET_64_MAX_ROWS, None      # (measure what the rule excludes too)
    for P, N, size, whats in shapes:
        torch.manual_seed(1)
        net = models.squiggle_predictor(size=size, depth=4, winlen=9).to(dev)
        bases = synth.randint(7, 1, P * N, 4).reshape(P, N)
        emb = torch.from_numpy(np.stack([squiggle_match.embed_sequence(bases[:, n], alphabet=None) for n in range(N)],
                                        axis=1)).to(dev)
        assert net.takes_operator(emb)
        dy = torch.randn(P, N, 3, device=dev)
        tag = dict(P=P, N=N, size=size, depth=4, winlen=9, rule_admits=size != 64 or rule is None or P * N <= rule)

        def fwd():
            with torch.no_grad():
                net(emb)

        def fwd_bwd():
            net.zero_grad(set_to_none=True)
            net(emb).backward(dy)

        # train_squiggle.py:216-223: about ten samples a position, levels near the prediction's scale
        siglen = torch.full((N,), 10 * P, dtype=torch.int64, device=dev)
        signal, nsample = torch.randn(int(siglen.sum()), device=dev), float(siglen.sum())

        def step():
            net.zero_grad(set_to_none=True)
            loss = squiggle_match.squiggle_match_loss(net(emb), signal, siglen, 1e-4)
            (loss.sum() / nsample).backward()

        for what in whats:
            if what == "step" and P > squiggle_match.MAX_NPOS:
                continue
            compare(dict(tag, what=what), {"fwd": fwd, "fwd+bwd": fwd_bwd, "step": step}[what], a)
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "launches": layers.SQUIGGLE_NET_LAUNCHES}))


if __name__ == "__main__":
    main()
