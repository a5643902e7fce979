#!/usr/bin/env python
"""LDS-array, VALU and matrix-core activity of the projection GEMMs (csrc/rnn_proj.hip, proj_kernel) from rocprofv3 PMC
passes, each a run of its own with nothing traced beside it (tools/lstm_fwd_counters.py has the pattern).

    python tools/proj_counters.py [--T 800] [--N 128] [--H 256] [--gates 4] [--reps 3] [--tree DIR]

--tree DIR takes taiyaki_amd (and its built libraries) from another checkout, e.g. the parent commit's, so that both
sides of a change are counted by the same tool.  The child makes --reps calls of tk_rnn_input_proj_dev and then --reps
of tk_rnn_input_grad_dev; proj_kernel's dispatches are told apart by their order.  Prints one JSON line: per form the
counters per launch (summed over the counters' instances, averaged over the launches) and per k block and workgroup
(per launch / (row tiles x column tiles x k blocks)); two workgroups share a CU, so a CU spends twice that per pair of
blocks.  The second pass (matrix-core counters) is reported as null where the device does not list them."""
import argparse
import csv
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PASSES = [["SQ_LDS_IDX_ACTIVE", "SQ_INSTS_LDS", "SQ_LDS_BANK_CONFLICT", "SQ_INSTS_VALU", "SQ_BUSY_CYCLES"],
          ["SQ_VALU_MFMA_BUSY_CYCLES", "SQ_INSTS_VALU_MFMA_MOPS_BF16", "SQ_WAVE_CYCLES"]]
RT, NT, KB = 128, 128, 16       # the kernel's tile (csrc/rnn_proj.hip)


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from taiyaki_amd import _lib, layers
    dev = torch.device("cuda:0")
    rows, H, G = a.T * a.N, a.H, a.gates * a.H
    g = torch.Generator(device="cpu").manual_seed(13)
    x = torch.randn(rows, H, generator=g).to(dev)
    dgt = torch.randn(rows, G, generator=g).to(dev)
    w = (torch.rand(G, H, generator=g) * 2 - 1).div_(H ** 0.5).to(dev)
    b = torch.randn(G, generator=g).to(dev)
    cus, P, p = layers._cu_count(dev), _lib.rnn_proj_lib(), _lib.ptr
    big = max(rows, 1 << 16)
    wsb = max(P.tk_rnn_proj_workspace_bytes(big, H, G, cus), P.tk_rnn_proj_workspace_bytes(big, G, H, cus))
    if min(P.tk_rnn_proj_workspace_bytes(big, H, G, cus), P.tk_rnn_proj_workspace_bytes(big, G, H, cus)) == 0:
        raise SystemExit("(H, gates) = (%d, %d) has no projection plan" % (H, a.gates))
    ws = torch.empty(wsb, dtype=torch.uint8, device=dev)
    gx, dx = torch.empty(rows, G, device=dev), torch.empty(rows, H, device=dev)
    for _ in range(a.reps):
        _lib.check(P.tk_rnn_input_proj_dev(p(x), p(w), p(b), rows, H, G, cus, p(gx), p(ws), wsb, _lib.stream_ptr()), "proj")
    torch.cuda.synchronize()
    for _ in range(a.reps):
        _lib.check(P.tk_rnn_input_grad_dev(p(dgt), p(w), rows, H, G, cus, p(dx), p(ws), wsb, _lib.stream_ptr()), "dx")
    torch.cuda.synchronize()
    print("cus %d" % cus)


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
    out = tempfile.mkdtemp(prefix="proj_pmc_", dir="/tmp")
    cmd = ["rocprofv3", "--pmc"] + counters + ["--output-format", "csv", "-d", out, "-o", "pmc", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--T", str(a.T), "--N", str(a.N), "--H", str(a.H), "--gates", str(a.gates),
           "--reps", str(a.reps), "--tree", os.path.abspath(a.tree)]
    pr = subprocess.run(cmd, capture_output=True, text=True, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=400)
    rows = read_csv(out) if pr.returncode == 0 else []
    shutil.rmtree(out, ignore_errors=True)
    if not rows:
        return None, (pr.stderr or pr.stdout)[-400:]
    # a dispatch's value: the sum over the counter's instances (one csv row each, or already summed)
    per = {}
    for name, disp, cname, val in rows:
        if "proj_kernel" in name and "prep" not in name:
            per[(disp, cname)] = per.get((disp, cname), 0.0) + val
    disps = sorted({d for d, _ in per})
    if len(disps) != 2 * a.reps:
        return None, "%d proj_kernel dispatches where %d were made" % (len(disps), 2 * a.reps)
    forms = {"proj": disps[:a.reps], "grad": disps[a.reps:]}
    res = {f: {c: sum(per[(d, c)] for d in ds) / len(ds) for c in counters if (ds[0], c) in per} for f, ds in forms.items()}
    return res, pr.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=800)
    ap.add_argument("--N", type=int, default=128)
    ap.add_argument("--H", type=int, default=256)
    ap.add_argument("--gates", type=int, default=4)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    if shutil.which("rocprofv3") is None:
        raise SystemExit("rocprofv3 is not on PATH")
    rows, H, G = a.T * a.N, a.H, a.gates * a.H
    blocks = {"proj": -(-rows // RT) * -(-G // NT) * (H // KB), "grad": -(-rows // RT) * -(-H // NT) * (G // KB)}
    per_launch = {"proj": {}, "grad": {}}
    failed = {}
    for i, counters in enumerate(PASSES):
        res, msg = one_pass(a, counters)
        if res is None:
            if i == 0:
                raise SystemExit("the counter pass failed: %s" % msg)
            failed = {c: None for c in counters}
            print("(the pass of %s failed: %s)" % (" ".join(counters), msg.strip()[-200:]), file=sys.stderr)
            continue
        for f in per_launch:
            per_launch[f].update(res[f])
    doc = {"tool": "tools/proj_counters.py", "T": a.T, "N": a.N, "H": a.H, "gates": a.gates, "reps": a.reps,
           "tree": os.path.abspath(a.tree), "blocks_x_workgroups": blocks,
           "per_launch": {f: dict(per_launch[f], **failed) for f in per_launch},
           "per_k_block_and_workgroup": {f: {c: round(v / blocks[f], 2) for c, v in per_launch[f].items()} for f in per_launch},
           "note": "per launch: summed over the counters' instances, mean of --reps launches; two workgroups share a CU, "
                   "so per CU and pair of blocks it is twice the per-workgroup figure; SQ_BUSY_CYCLES and the other "
                   "*_CYCLES are summed over their instances like the rest"}
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
