#!/usr/bin/env python
"""Times the alignment kernels of include/taiyaki_amd_align.h (taiyaki_amd/accuracy.py).  Three records, one JSON line each:

validation   --calls calls at T --blocks with labels of realistic length (synth.realistic_seqlens) on scores that follow
             the labels with --noise: the launch of tk_align_calls_dev beside the Viterbi launch of the same batch, the
             whole `call_accuracy`, and the host chain on the same machine (download of the path, collapse, the numpy
             row sweep of tests/align_support.py's kind).
long_reads   --pairs pairs of 10 000 .. 50 000 codes at --rate mutation through `align_pairs_exact`: rounds, the largest
             max_distance reached, milliseconds (upload, launches and the per-round reads included).
per_cell     one launch of 256 pairs of 2000 x 2000 codes at a band of each cells-per-lane count (tk_align_band names
             it): nanoseconds per row of a wave and per cell.

    python tools/alignbench.py [--steps 20] [--warmup 3]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from taiyaki_amd import _lib, accuracy, decode, synth  # noqa: E402

BIG = 1 << 32


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


def host_sweep(q, r):
    """(D, M): the recurrence a row per numpy step"""
    ramp = np.arange(len(r) + 1, dtype=np.int64) * BIG
    row = ramp.copy()
    for i in range(1, len(q) + 1):
        new = np.empty_like(row)
        new[0] = i * BIG
        new[1:] = np.minimum(row[:-1] + np.where(r == q[i - 1], -1, BIG), row[1:] + BIG)
        row = np.minimum.accumulate(new - ramp) + ramp
    key = int(row[-1])
    d = -(-key // BIG)
    return d, d * BIG - key


def mutate(seq, rate, rng):
    u = rng.random_sample(len(seq))
    sub, ins, dele = u < rate / 3, (u >= rate / 3) & (u < 2 * rate / 3), (u >= 2 * rate / 3) & (u < rate)
    out = np.where(sub, (seq + 1 + rng.randint(3, size=len(seq))) % 4, seq).astype(np.uint8)
    pieces = np.stack([out, rng.randint(4, size=len(seq)).astype(np.uint8)], axis=1)
    keep = np.stack([~dele, ins], axis=1)
    return pieces[keep]


def validation(a, dev):
    T, N = a.blocks, a.calls
    seqlens = synth.realistic_seqlens(T, N, 40, 5 * T, 9.0)
    inp = synth.confident_scores(synth.crf_case(T, N, 41, seqlens=seqlens), 42, noise=a.noise)
    sc = torch.from_numpy(inp["scores"]).to(dev)
    seqs, lens = torch.from_numpy(inp["seqs"]), torch.from_numpy(inp["seqlens"].astype(np.int64))
    res = accuracy.call_alignment(sc, seqs, lens)
    path = decode.flipflop_viterbi_path(sc)
    # the alignment launch alone, on tensors made once
    seqs_d = seqs.to(dev, torch.int32)
    lens_d = lens.to(dev, torch.int32)
    off_d = torch.from_numpy(np.concatenate([[0], np.cumsum(inp["seqlens"])]).astype(np.int64)).to(dev)
    out = [torch.zeros(N, dtype=torch.int32, device=dev) for _ in range(3)]
    widest = T + 2 + int(inp["seqlens"].max())
    L, p = _lib.align_lib(), _lib.ptr

    def launch():
        _lib.check(L.tk_align_calls_dev(p(path), None, T, N, 4, p(seqs_d), p(off_d), p(lens_d), widest, p(out[0]), p(out[1]),
                                        p(out[2]), _lib.stream_ptr()), "tk_align_calls_dev")

    align_us = 1e3 * timed(launch, a.steps, a.warmup)
    assert all(torch.equal(o, r) for o, r in zip(out, (res.distance, res.matches, res.exact)))
    viterbi_us = 1e3 * timed(lambda: decode.flipflop_viterbi_path(sc), a.steps, a.warmup)
    whole_us = 1e3 * timed(lambda: accuracy.call_accuracy(sc, seqs, lens), a.steps, a.warmup)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    host_path = path.cpu().numpy()
    t1 = time.perf_counter()
    want, at = [], 0
    for n in range(N):
        col = host_path[:, n]
        call = (col[np.ediff1d(col, to_begin=1) != 0] % 4).astype(np.uint8)
        want.append(host_sweep(call, (inp["seqs"][at:at + inp["seqlens"][n]] % 4).astype(np.uint8)))
        at += inp["seqlens"][n]
    t2 = time.perf_counter()
    assert [tuple(w) for w in want] == list(zip(res.distance.tolist(), res.matches.tolist()))
    ncall = (res.columns - res.distance).float().mean().item()
    return dict(record="validation", T=T, N=N, mean_labels=float(inp["seqlens"].mean()), mean_matches=ncall,
                mean_accuracy=accuracy.summary(res.accuracy)["mean"], align_launch_us=round(align_us, 1),
                viterbi_launch_us=round(viterbi_us, 1), call_accuracy_us=round(whole_us, 1),
                host_download_us=round(1e6 * (t1 - t0), 1), host_sweep_us=round(1e6 * (t2 - t1), 1))


def long_reads(a, dev):
    rng = np.random.RandomState(43)
    refs = [rng.randint(4, size=n).astype(np.uint8) for n in rng.randint(10000, 50001, size=a.pairs)]
    queries = [mutate(r, a.rate, rng) for r in refs]
    accuracy.align_pairs_exact(queries[:2], refs[:2])        # (loads the library, warms the allocator)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    res = accuracy.align_pairs_exact(queries, refs)
    torch.cuda.synchronize()
    ms = 1e3 * (time.perf_counter() - t0)
    assert bool(res.exact.all())
    return dict(record="long_reads", pairs=a.pairs, rate=a.rate, codes=int(sum(len(r) for r in refs)),
                rounds=accuracy.last_exact["rounds"], max_distance=accuracy.last_exact["max_distance"],
                ms=round(ms, 1), mean_distance=res.distance.float().mean().item(),
                mean_accuracy=accuracy.summary(res.accuracy)["mean"])


def per_cell(a, dev):
    rng = np.random.RandomState(44)
    npair, n = 256, 2000
    refs = [rng.randint(4, size=n).astype(np.uint8) for _ in range(npair)]
    queries = [r.copy() for r in refs]
    pk = accuracy._Pairs(queries, refs, "alignbench").upload()
    out = accuracy._empty_out(npair, pk.device)
    rows = []
    for cells in (1, 2, 4, 8, 16, 17, 33, 63):
        t = 64 * cells - 2                       # a band of 64 cells - 1 diagonals
        got = [ctypes.c_int() for _ in range(3)]
        assert _lib.align_lib().tk_align_band(n, n, t, *[ctypes.byref(g) for g in got]) == 0 and got[2].value == cells
        width = got[1].value - got[0].value + 1
        ms = timed(lambda: pk.launch(out, None, t, width), a.steps, a.warmup)
        assert out[0].sum().item() == 0 and out[1].sum().item() == npair * n
        rows.append(dict(cells_per_lane=cells, band=width, where="registers" if cells <= 16 else "LDS",
                         launch_us=round(1e3 * ms, 1), ns_per_row=round(1e6 * ms / n, 1),
                         ns_per_cell_of_a_wave=round(1e6 * ms / (n * width), 3),
                         ns_per_cell_of_the_launch=round(1e6 * ms / (n * width * npair), 4)))
    return dict(record="per_cell", pairs=npair, rows_per_pair=n, by_cells_per_lane=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--calls", type=int, default=128)
    ap.add_argument("--blocks", type=int, default=800)
    ap.add_argument("--noise", type=float, default=4.0)
    ap.add_argument("--pairs", type=int, default=64)
    ap.add_argument("--rate", type=float, default=0.1)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("alignbench needs a GPU (the alignment has no CPU fallback)")
    dev = torch.device("cuda:0")
    # the validation record once more on scores that ignore the labels: the worst case of the band that grows in the wave
    records = [validation, lambda a, dev: dict(validation(argparse.Namespace(**dict(vars(a), noise=40.0)), dev),
                                               record="validation_random_calls"), long_reads, per_cell]
    for record in records:
        print(json.dumps(dict(record(a, dev), device=torch.cuda.get_device_name(dev))), flush=True)


if __name__ == "__main__":
    main()
