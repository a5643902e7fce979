#!/usr/bin/env python
"""Times one `GruMod(256, 256)` under no_grad on the matrix cores (csrc/gru_matrix_group.hip: groups of 4 workgroups,
slabs inside the entry) against what runs the same call with the switch off: the kernels of the main library, beyond 256
columns as slabs (csrc/gru_kernels.hip; with lengths its build of include/taiyaki_amd_rnn_varlen.h).  The input
projection is part of both sides.

Every (T, N) of --shapes is warmed up on both sides first.  Then, for every shape, with full lengths (none given) and
with lengths spread evenly over T/4 ... T: layers.USE_HIP_GRU_MATRIX_GROUP off and on in turns in one process (threshold
1), each timed with device events (median over --steps), --turns turns.  One JSON line per case: microseconds per call
and turn, whether the new kernel was ahead in EVERY turn, and the largest difference of the two outputs.  Then one JSON
line with the threshold the table sets: the smallest measured N from which the new kernel is ahead in every turn, there
and at every larger N measured, with both kinds of lengths (null: there is none).

--basecall: one whole `Basecaller.call` on a seeded mGru_flipflop of size 256 at max_concurrent_chunks 2048 and 4096,
switch off and on in turns (the threshold as shipped unless --min-columns): samples per second and the reads whose calls
are equal on both sides.

    python tools/grumatrixgroupbench.py [--shapes 800x512,...] [--steps 5] [--warmup 2] [--turns 3]
    python tools/grumatrixgroupbench.py --basecall [--reads 384] [--min-columns 513]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import layers  # noqa: E402

H = 256
SHAPES = ",".join("800x%d" % N for N in (512, 1024, 2048, 4096, 8192))
SIDES = ("parent", "group")


def case(T, N, spread, dev):
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(T, N, H, generator=g, device=dev)
    lens = None
    if spread:
        lens = torch.linspace(T // 4, T, N, device=dev).round().to(torch.int32)[torch.randperm(N, generator=g, device=dev)]
        lens = lens.contiguous()
    return x, lens


def leg(gru, x, lens, side):
    layers.USE_HIP_GRU_MATRIX_GROUP = side == "group"
    before = layers.gru_matrix_group_calls["inference"]
    y = gru(x, lengths=lens)
    assert (layers.gru_matrix_group_calls["inference"] != before) == (side == "group"), side
    return y


def timed(fn, steps):
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def layer_turns(gru, T, N, spread, turns, steps, dev):
    x, lens = case(T, N, spread, dev)
    out = {k: [] for k in SIDES}
    for _ in range(turns):
        for side in SIDES:
            out[side].append(round(1e3 * timed(lambda: leg(gru, x, lens, side), steps), 1))
    ys = {side: leg(gru, x, lens, side) for side in SIDES}
    return {"T": T, "N": N, "lengths": "spread" if spread else "full", "us_per_call": out,
            "us_per_step_median": {k: round(float(np.median(v)) / T, 3) for k, v in out.items()},
            "group_ahead_every_turn": all(a < b for a, b in zip(out["group"], out["parent"])),
            "max_abs_diff": (ys["group"] - ys["parent"]).abs().max().item()}


def basecall_turns(turns, reads, chunks, dev):
    from taiyaki_amd import basecall, models, synth
    rs = np.random.RandomState(9)
    sigs = [(90 + 12 * rs.standard_normal(int(n))).astype(np.float32) for n in rs.randint(20000, 100001, size=reads)]
    torch.manual_seed(17)
    net = synth.excite_network(models.mGru_flipflop(size=H)).to(dev).eval()
    caller = basecall.Basecaller(net, fastq=True, max_concurrent_chunks=chunks)
    nsamples = sum(len(s) for s in sigs)
    out, calls, seqs = {"off": [], "on": []}, {}, {}
    for turn in range(turns + 1):           # (the first turn is the warm-up at the timed shapes)
        for side in out:
            layers.USE_HIP_GRU_MATRIX_GROUP = side == "on"
            before = layers.gru_matrix_group_calls["inference"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = caller.call(sigs)         # (ends in its download)
            dt = time.perf_counter() - t0
            calls[side] = layers.gru_matrix_group_calls["inference"] - before
            seqs[side] = [r[0] for r in res]
            if turn:
                out[side].append(round(nsamples / dt))
    same = sum(a == b for a, b in zip(seqs["off"], seqs["on"]))
    return {"basecall": "mGru_flipflop 256, %d reads, %d samples, max_concurrent_chunks %d" % (len(sigs), nsamples, chunks),
            "min_columns": layers.GRU_MATRIX_GROUP_MIN_COLUMNS, "samples_per_s": out, "group_launches_per_call": calls,
            "reads_with_equal_calls": "%d / %d" % (same, len(sigs)), "bases": sum(len(s) for s in seqs["on"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="T x N, comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--basecall", action="store_true")
    ap.add_argument("--reads", type=int, default=384)
    ap.add_argument("--min-columns", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grumatrixgroupbench needs a GPU (the recurrence has no CPU fallback)")
    dev = torch.device("cuda:0")
    shipped = layers.USE_HIP_GRU_MATRIX_GROUP
    if a.basecall:
        if a.min_columns:
            layers.GRU_MATRIX_GROUP_MIN_COLUMNS = a.min_columns
        for chunks in (2048, 4096):
            print(json.dumps(basecall_turns(a.turns, a.reads, chunks, dev)), flush=True)
        return
    layers.GRU_MATRIX_GROUP_MIN_COLUMNS = 1         # (the table is what sets the shipped value)
    torch.manual_seed(3)
    gru = layers.GruMod(H, H).to(dev)
    shapes = [tuple(int(v) for v in shape.split("x")) for shape in a.shapes.split(",")]
    ahead = {}
    with torch.no_grad():
        for T, N in shapes:
            for spread in (False, True):
                x, lens = case(T, N, spread, dev)
                for _ in range(a.warmup):
                    for side in SIDES:
                        leg(gru, x, lens, side)
        torch.cuda.synchronize()
        for T, N in shapes:
            for spread in (False, True):
                row = layer_turns(gru, T, N, spread, a.turns, a.steps, dev)
                ahead[N] = ahead.get(N, True) and row["group_ahead_every_turn"]
                print(json.dumps(row), flush=True)
    widths = sorted(ahead)
    from_n = [n for i, n in enumerate(widths) if all(ahead[m] for m in widths[i:])]
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "cus": layers._cu_count(dev), "switch_as_shipped": shipped,
                      "ahead_with_both_kinds_of_lengths": ahead, "threshold": from_n[0] if from_n else None}), flush=True)


if __name__ == "__main__":
    main()
