#!/usr/bin/env python
"""VALU, LDS-array and matrix-core activity of the weight-gradient kernel (csrc/wgrad_common.h, wgrad_kernel) from
rocprofv3 PMC passes, each a run of its own with nothing traced beside it (tools/proj_counters.py has the pattern).

    python tools/wgrad_counters.py [--cell lstm|gru] [--T 800] [--N 128] [--H 256] [--reps 3] [--tree DIR]

--tree DIR takes taiyaki_amd (and its built libraries) from another checkout, e.g. the parent commit's, so that both
sides of a change are counted by the same tool.  The child makes --reps calls of tk_<cell>_weight_grad_dev at
(T, N, H, I = H) and prints its plan.  Prints one JSON line: the counters per launch of wgrad_kernel (summed over the
counters' instances, averaged over the launches) and per block and tile: per launch / (output tiles of 128 x 128 x
blocks of 16 rows), the unit of work that is the same whichever workgroup does it (a square workgroup does one per
barrier, a tall one two).  The second pass (matrix-core counters) is reported as null where the device does not list
them."""
import argparse
import csv
import ctypes
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = [["SQ_LDS_IDX_ACTIVE", "SQ_INSTS_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_INSTS_VALU", "SQ_BUSY_CYCLES"],
          ["SQ_VALU_MFMA_BUSY_CYCLES", "SQ_INSTS_VALU_MFMA_MOPS_BF16", "SQ_WAVE_CYCLES"]]
KB = 16         # rows per block (csrc/wgrad_common.h, WG_KB)
GATES = {"lstm": 4, "gru": 3}


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from taiyaki_amd import _lib, layers
    dev = torch.device("cuda:0")
    T, N, H, G = a.T, a.N, a.H, GATES[a.cell] * a.H
    g = torch.Generator(device="cpu").manual_seed(17)
    dg = torch.randn(T, N, G, generator=g).to(dev)
    dq = torch.randn(T, N, H, generator=g).to(dev)
    x = torch.randn(T, N, H, generator=g).to(dev)
    y = torch.randn(T, N, H, generator=g).to(dev)
    cus, p = layers._cu_count(dev), _lib.ptr
    dw_ih, dw_hh = torch.empty(G, H, device=dev), torch.empty(G, H, device=dev)
    db, db2 = torch.empty(G, device=dev), torch.empty(G, device=dev)
    if a.cell == "lstm":
        W = _lib.wgrad_lib()
        wsb = W.tk_lstm_weight_grad_workspace_bytes(T, N, H, H, cus)
        lab = _lib._load(os.path.join(_lib.CSRC, _lib.WGRAD_LAB_LIBNAME), dict(_lib.WGRAD_SIGNATURES, **_lib.WGRAD_LAB_SIGNATURES))
    else:
        W = _lib.gru_wgrad_lib()
        wsb = W.tk_gru_weight_grad_workspace_bytes(T, N, H, H, cus)
        lab = _lib._load(os.path.join(_lib.CSRC, _lib.GRU_WGRAD_LAB_LIBNAME),
                         dict(_lib.GRU_WGRAD_SIGNATURES, **_lib.GRU_WGRAD_LAB_SIGNATURES))
    if wsb == 0:
        raise SystemExit("(T, N, H) = (%d, %d, %d) has no weight-gradient plan" % (T, N, H))
    plan = (ctypes.c_size_t * 8)()
    assert getattr(lab, "tk_lab_%s_wgrad_plan" % a.cell)(T, N, H, H, cus, plan)
    ws = torch.empty(wsb // 4, device=dev)
    for _ in range(a.reps):
        if a.cell == "lstm":
            rc = W.tk_lstm_weight_grad_dev(p(dg), p(x), p(y), T, N, H, H, 0, cus, p(dw_ih), p(dw_hh), p(db), p(ws), wsb,
                                           _lib.stream_ptr())
        else:
            rc = W.tk_gru_weight_grad_dev(p(dg), p(dq), p(x), p(y), T, N, H, H, 0, cus, p(dw_ih), p(dw_hh), p(db), p(db2),
                                          p(ws), wsb, _lib.stream_ptr())
        _lib.check(rc, "weight_grad")
    torch.cuda.synchronize()
    print("plan %s cus %d" % (" ".join(str(v) for v in plan), cus))


def read_csv(outdir):
    """[(kernel name, dispatch id, counter, value)] from every counter_collection csv under outdir."""
    rows = []
    for dp, _, fs in os.walk(outdir):
        for f in fs:
            if f.endswith("counter_collection.csv"):
                with open(os.path.join(dp, f), newline="") as fh:
                    for r in csv.DictReader(fh):
                        rows.append((r["Kernel_Name"], int(r["Dispatch_Id"]), r["Counter_Name"], float(r["Counter_Value"])))
    return rows


def one_pass(a, counters):
    out = tempfile.mkdtemp(prefix="wgrad_pmc_", dir="/tmp")
    cmd = ["rocprofv3", "--pmc"] + counters + ["--output-format", "csv", "-d", out, "-o", "pmc", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--cell", a.cell, "--T", str(a.T), "--N", str(a.N), "--H", str(a.H),
           "--reps", str(a.reps), "--tree", os.path.abspath(a.tree)]
    pr = subprocess.run(cmd, capture_output=True, text=True, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=400)
    rows = read_csv(out) if pr.returncode == 0 else []
    shutil.rmtree(out, ignore_errors=True)
    if not rows:
        return None, None, (pr.stderr or pr.stdout)[-400:]
    # a dispatch's value: the sum over the counter's instances (one csv row each, or already summed)
    per, names = {}, set()
    for name, disp, cname, val in rows:
        if "wgrad_kernel" in name:
            per[(disp, cname)] = per.get((disp, cname), 0.0) + val
            names.add(name)
    disps = sorted({d for d, _ in per})
    if len(disps) != a.reps:
        return None, None, "%d wgrad_kernel dispatches where %d were made" % (len(disps), a.reps)
    res = {c: sum(per[(d, c)] for d in disps) / len(disps) for c in counters if (disps[0], c) in per}
    plan = [ln for ln in pr.stdout.splitlines() if ln.startswith("plan ")]
    return res, (sorted(names), plan[-1] if plan else None), pr.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cell", choices=sorted(GATES), default="lstm")
    ap.add_argument("--T", type=int, default=800)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if shutil.which("rocprofv3") is None:
        raise SystemExit("rocprofv3 is not on PATH")
    per_launch, failed, seen = {}, {}, None
    for i, counters in enumerate(PASSES):
        res, info, msg = one_pass(a, counters)
        if res is None:
            if i == 0:
                raise SystemExit("the counter pass failed: %s" % msg)
            failed = {c: None for c in counters}
            print("(the pass of %s failed: %s)" % (" ".join(counters), msg.strip()[-200:]), file=sys.stderr)
            continue
        per_launch.update(res)
        seen = seen or info
    names, plan_line = seen
    units = None
    if plan_line:
        v = [int(s) for s in plan_line.split()[1:9]]
        tiles_m, tiles_n, runs, parts, run_rows, part_rows = v[:6]
        K, blocks = a.T * a.N, 0
        for r in range(runs):
            end = min((r + 1) * run_rows, K)
            for s in range(parts):
                k0 = r * run_rows + s * part_rows
                blocks += max(0, -(-(min(k0 + part_rows, end) - k0) // KB))
        units = tiles_m * tiles_n * blocks
    doc = {"tool": "tools/wgrad_counters.py", "cell": a.cell, "T": a.T, "N": a.N, "H": a.H, "reps": a.reps,
           "tree": os.path.abspath(a.tree), "kernels": names, "plan": plan_line, "blocks_x_tiles": units,
           "per_launch": dict(per_launch, **failed),
           "per_block_and_tile": {c: round(v / units, 2) for c, v in per_launch.items()} if units else None,
           "note": "per launch: summed over the counters' instances, mean of --reps launches; a block and tile is 16 rows "
                   "of one 128 x 128 output tile: 12 MFMAs of 32 cycles on each of the 8 waves that share it; "
                   "SQ_BUSY_CYCLES and the other *_CYCLES are summed over their instances like the rest"}
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
