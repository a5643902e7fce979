#!/usr/bin/env python
"""LDS-array and VALU activity of the LSTM forward recurrence (csrc/lstm_kernels.hip, lstm_fwd_kernel) from ONE
rocprofv3 PMC pass in a run of its own, nothing else traced beside the kernel names (tools/sq_counters.py has the
pattern; the rocpd database is read with its `read`).

    python tools/lstm_fwd_counters.py [--T 800] [--N 128] [--H 256] [--reps 3] [--tree DIR]

--tree DIR takes taiyaki_amd (and its built libraries) from another checkout, e.g. the parent commit's, so that both
sides of a change are counted by the same tool.  Prints one JSON line: the counters per launch (summed over the
counters' instances, averaged over --reps launches), and per step and workgroup (one workgroup per CU) the LDS-array
cycles, bank-conflict cycles and LDS / VALU wave-instructions, next to what the kernel's instruction counts predict."""
import argparse
import json
import os
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COUNTERS = ["SQ_LDS_IDX_ACTIVE", "SQ_LDS_BANK_CONFLICT", "SQ_INSTS_LDS", "SQ_INSTS_VALU", "SQ_ACTIVE_INST_LDS",
            "SQ_BUSY_CYCLES"]


def child(a):
    sys.path.insert(0, os.path.abspath(a.tree))
    import torch
    from taiyaki_amd import _lib, layers
    dev = torch.device("cuda:0")
    T, N, H = a.T, a.N, a.H
    g = torch.Generator(device="cpu").manual_seed(11)
    w_hh = (torch.rand(4 * H, H, generator=g) * 2 - 1).div_(H ** 0.5).to(dev)
    gx = torch.randn(T, N, 4 * H, generator=g).to(dev)
    y, gates, cell = torch.empty(T, N, H, device=dev), torch.empty(T, N, 4 * H, device=dev), torch.empty(T, N, H, device=dev)
    cus, L, P = layers._cu_count(dev), _lib.lib(), _lib.ptr
    wsb = L.tk_lstm_workspace_bytes(N, H, cus)
    if wsb == 0:
        raise SystemExit("(N, H) = (%d, %d) is not admitted on %d CUs" % (N, H, cus))
    ws, status = torch.empty(wsb // 4, dtype=torch.float32, device=dev), _lib.status_word(dev)
    for _ in range(a.reps):
        _lib.check(L.tk_lstm_forward_dev(P(gx), P(w_hh), T, N, H, 0, cus, P(y), P(gates), P(cell), P(ws), wsb,
                                         P(status), _lib.stream_ptr()), "tk_lstm_forward_dev")
    torch.cuda.synchronize()
    _lib.finish(status)
    print("cus %d" % cus)


def main():
    ap = argparse.ArgumentParser()
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
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import sq_counters
    out = tempfile.mkdtemp(prefix="lstm_fwd_pmc_", dir="/tmp")
    cmd = ["rocprofv3", "--kernel-trace", "--pmc"] + COUNTERS + ["-d", out, "-o", "pmc", "--", sys.executable,
           os.path.abspath(__file__), "--child", "--T", str(a.T), "--N", str(a.N), "--H", str(a.H), "--reps", str(a.reps),
           "--tree", os.path.abspath(a.tree)]
    pr = subprocess.run(cmd, capture_output=True, text=True, cwd="/tmp", env=dict(os.environ, TMPDIR="/tmp"), timeout=400)
    dbs = [os.path.join(dp, f) for dp, _, fs in os.walk(out) for f in fs if f.endswith(".db")]
    if pr.returncode != 0 or not dbs:
        raise SystemExit("the counter pass failed (rc %d): %s" % (pr.returncode, (pr.stderr or pr.stdout)[-600:]))
    acc, kernel = {}, None
    for name, _disp, cname, val in sq_counters.read(dbs[0]):
        if "lstm_fwd_kernel" in name:
            kernel = name
            acc.setdefault(cname, []).append(float(val))
    shutil.rmtree(out, ignore_errors=True)
    if not acc:
        raise SystemExit("no lstm_fwd_kernel launch in the database")
    per_launch = {k: sum(v) / len(v) for k, v in sorted(acc.items())}
    cus = int(pr.stdout.strip().split("cus ")[-1].split()[0])
    # (N, H) = (128, 256) on 256 CUs: 8 admitted columns, U 64, C 2, one workgroup of 8 waves per CU; the matvec runs
    # in all T steps, the poll and the gather in T - 1 of them
    per = lambda k: per_launch.get(k, float("nan")) / (cus * max(a.T, 1))     # noqa: E731
    print(json.dumps({"tool": "tools/lstm_fwd_counters.py", "T": a.T, "N": a.N, "H": a.H, "tree": os.path.abspath(a.tree),
                      "kernel": kernel[:90], "launches": len(next(iter(acc.values()))), "cus": cus,
                      "per_launch": per_launch, "per_step_and_cu": {k: round(per(k), 2) for k in per_launch},
                      "note": "per_step_and_cu = per launch / (CUs x T), a grid of one workgroup per CU assumed; "
                              "SQ_BUSY_CYCLES is summed over its instances like the others"}))


if __name__ == "__main__":
    main()
