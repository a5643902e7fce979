#!/usr/bin/env python
"""Times one `GruMod(96, 96)` under no_grad with the matrix-core recurrence (csrc/gru_matrix.hip, 16 columns per
workgroup) against the same call on the kernels in use without it (csrc/gru_kernels.hip, 2 columns per workgroup at these
widths; with lengths its build of include/taiyaki_amd_rnn_varlen.h).  The input projection is part of both sides.

For every (T, N) of --shapes, with full lengths (no lengths given) and with lengths spread evenly over T/4 ... T:
layers.USE_HIP_GRU_MATRIX on and off in turns in one process, each timed with device events after warm-up (median over
--steps), --turns turns.  One JSON line per case: microseconds per call and turn, whether the matrix kernel was ahead in
EVERY turn, and the largest difference of the two outputs.  Then one JSON line with the threshold the table sets: the
smallest measured N from which the matrix kernel is ahead in every turn, there and at every larger N measured, at every
T and with both kinds of lengths (null: there is none).

--ut 1 or 2: the lab build with that many unit tiles per wave (6 or 3 waves per workgroup); the default is the release
library.  --basecall: one whole `Basecaller.call` on a seeded mGru_flipflop of size 96 at --chunks
max_concurrent_chunks, switch off and on in turns (the threshold as shipped unless --min-columns), samples per second.

    python tools/grumatrixbench.py [--shapes 200x512,...] [--steps 5] [--warmup 2] [--turns 3] [--ut 2] [--basecall]
"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, layers  # noqa: E402

H = 96
SHAPES = ",".join("%dx%d" % (T, N) for T in (200, 800) for N in (512, 1024, 2048, 4096, 8192))


def timed(fn, steps, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times))


def layer_turns(gru, T, N, spread, turns, steps, warmup, dev):
    g = torch.Generator(device=dev).manual_seed(11)
    x = torch.randn(T, N, H, generator=g, device=dev)
    lens = None
    if spread:
        lens = torch.linspace(T // 4, T, N, device=dev).round().to(torch.int32)[torch.randperm(N, generator=g, device=dev)]
        lens = lens.contiguous()
    ys, out = {}, {"matrix": [], "existing": []}

    def leg(side):
        layers.USE_HIP_GRU_MATRIX = side == "matrix"
        before = layers.gru_matrix_calls["inference"]
        ys[side] = gru(x, lengths=lens)
        assert (layers.gru_matrix_calls["inference"] != before) == (side == "matrix"), side

    for _ in range(turns):
        for side in out:
            out[side].append(round(1e3 * timed(lambda: leg(side), steps, warmup), 1))
    diff = (ys["matrix"] - ys["existing"]).abs().max().item()
    return {"T": T, "N": N, "lengths": "spread" if spread else "full", "us_per_call": out,
            "us_per_step_median": {k: round(float(np.median(v)) / T, 3) for k, v in out.items()},
            "matrix_ahead_every_turn": all(m < e for m, e in zip(out["matrix"], out["existing"])),
            "max_abs_diff": diff}


def basecall_turns(turns, chunks, dev):
    from taiyaki_amd import basecall, models, synth
    rs = np.random.RandomState(9)
    sigs = [(90 + 12 * rs.standard_normal(40000)).astype(np.float32) for _ in range(512)]
    torch.manual_seed(17)
    net = synth.excite_network(models.mGru_flipflop(size=H)).to(dev).eval()
    caller = basecall.Basecaller(net, fastq=True, max_concurrent_chunks=chunks)
    nsamples = sum(len(s) for s in sigs)
    out, calls, seqs = {"off": [], "on": []}, {}, {}
    for turn in range(turns + 1):           # (the first turn is the warm-up at the timed shapes)
        for side in out:
            layers.USE_HIP_GRU_MATRIX = side == "on"
            before = layers.gru_matrix_calls["inference"]
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = caller.call(sigs)         # (ends in its download)
            dt = time.perf_counter() - t0
            calls[side] = layers.gru_matrix_calls["inference"] - before
            seqs[side] = [r[0] for r in res]
            if turn:
                out[side].append(round(nsamples / dt))
    same = sum(a == b for a, b in zip(seqs["off"], seqs["on"]))
    return {"basecall": "mGru_flipflop 96, 512 reads x 40000 samples, max_concurrent_chunks %d" % chunks,
            "min_columns": layers.GRU_MATRIX_MIN_COLUMNS, "samples_per_s": out, "matrix_launches_per_call": calls,
            "reads_with_equal_calls": "%d / %d" % (same, len(sigs)), "bases": sum(len(s) for s in seqs["on"])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default=SHAPES, help="T x N, comma separated")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--turns", type=int, default=3)
    ap.add_argument("--ut", type=int, choices=(1, 2), default=0)
    ap.add_argument("--basecall", action="store_true")
    ap.add_argument("--chunks", default="2048,4096")
    ap.add_argument("--min-columns", type=int, default=0)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grumatrixbench needs a GPU (the recurrence has no CPU fallback)")
    dev = torch.device("cuda:0")
    if a.ut:
        os.environ["TK_LAB_GRU_MATRIX_UT"] = str(a.ut)
        assert _lib.use_lab(True)
    if a.basecall:
        if a.min_columns:
            layers.GRU_MATRIX_MIN_COLUMNS = a.min_columns
        for chunks in a.chunks.split(","):
            print(json.dumps(basecall_turns(a.turns, int(chunks), dev)), flush=True)
        return
    layers.GRU_MATRIX_MIN_COLUMNS = 1       # (the table is what sets the shipped value)
    torch.manual_seed(3)
    gru = layers.GruMod(H, H).to(dev)
    ahead = {}
    with torch.no_grad():
        for shape in a.shapes.split(","):
            T, N = (int(v) for v in shape.split("x"))
            for spread in (False, True):
                row = layer_turns(gru, T, N, spread, a.turns, a.steps, a.warmup, dev)
                ahead[N] = ahead.get(N, True) and row["matrix_ahead_every_turn"]
                print(json.dumps(row), flush=True)
    widths = sorted(ahead)
    from_n = [n for i, n in enumerate(widths) if all(ahead[m] for m in widths[i:])]
    print(json.dumps({"device": torch.cuda.get_device_name(dev), "cus": layers._cu_count(dev), "unit_tiles_per_wave":
                      a.ut or "release", "ahead_at_every_T_and_lengths": ahead,
                      "threshold": from_n[0] if from_n else None}), flush=True)


if __name__ == "__main__":
    main()
