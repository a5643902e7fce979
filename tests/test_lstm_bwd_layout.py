"""The block layout of the LSTM backward's matvec (csrc/lstm_bwd_layout.h; lstm_bwd_kernel at H 256, U 64): a lane
holds KQ = 4 columns of W_hh over 32 owned rows, the 8 lanes that share those columns add their partial sums inside the
wave by recursive halving, and each lane publishes the sums it is left with.

CPU: the header compiled for the host and enumerated -- every owned weight in exactly one lane, every (k, c) sum
published by exactly one lane, the rows of a lane and the tree the same at 2 and at 4 columns, and the halving, run
lane by lane in numpy, leaving the sums the header says where it says.

GPU, at the C ABI, both instantiations ((256, 64, 2) at N = 15, (256, 64, 4) at 8 (CUs // 16) + 1 columns: ragged last
groups), T <= 7, both directions, with and without lengths:
  * dgates between guards over a sentinel against the float64 recurrence's gradient on a random dense W_hh (a misplaced
    weight is an O(1) error), inside 2 x MIOpen's own error + 2e-6 (the rule of tests/test_rnn_instantiations.py; with
    lengths, MIOpen's error at full length);
  * dy non-zero in one (t, n, unit) per column, at the recurrence's first step, the units one per workgroup member and
    per lane residue rq of the row partition: dgates of the next step, a four-term sum per k, within 1e-6 of its largest
    entry of float64 (fp32 rounds each of the handful of operations behind an entry to 6e-8);
  * two calls, the same bits; a column of the 4-column launch, the same bits in a 2-column launch of the same data;
    the plain pair, the lab build, lengths = NULL and lengths = [T] * N of the variable-length build, and the wide
    build, the same bits.

What the across-columns case found when it was written: with the column layout the 4-column launch's gather added the
four producers as (0 + 2) + (1 + 3) and the 2-column launch's as ((0 + 1) + 2) + 3, and a column's dgates differed by
7.5e-9 between the two; the gather of these two instantiations now adds in producer order at either width.
profiles/r35_lstm_bwd_layout.txt keeps the errors beside MIOpen's.

After a non-zero status word or return code this module launches nothing more."""
import functools
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib
from tests import test_lstm_fwd_rows as rows
from tests import test_rnn_instantiations as insts

H, U, NT = 256, 64, 512
INSTS = [(256, 64, 2), (256, 64, 4)]
HEADER = os.path.join(_lib.CSRC, "lstm_bwd_layout.h")
_ids = insts._ids


# ---------------------------------------------------------------------------------------------------------------------
# CPU: the header, enumerated
# ---------------------------------------------------------------------------------------------------------------------
_PROGRAM = r"""
#include <cstdio>
#include "%s"
int main() {
    const int cases[][4] = {{512, 256, 64, 2}, {512, 256, 64, 4}};
    for (auto &c : cases) {
        const tk::LstmBwdBlock b(c[0], c[1], c[2], c[3]);
        std::printf("block %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", b.NT, b.H, b.U, b.C, b.KQ, b.RQ, b.RR, b.KEEP, (int)b.ok());
        for (int rq = 0; rq < b.RQ; ++rq) {
            std::printf("lane %%d %%d", rq, b.kept_first(rq));
            for (int j = 0; j < b.RR; ++j) std::printf(" %%d", b.row(rq, j));
            std::printf("\n");
        }
    }
    const int others[][2] = {{16, 16}, {32, 16}, {32, 32}, {64, 16}, {64, 32}, {64, 64}, {128, 16}, {128, 32}, {128, 64},
                             {256, 16}, {256, 32}, {192, 48}, {384, 48}};
    for (auto &o : others) std::printf("kq %%d %%d %%d\n", o[0], o[1], tk::lstm_bwd_kq(o[0], o[1]));
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _enumerated():
    """{C: (fields, {rq: (kept_first, rows)})} and {(H, U): KQ} from the header, compiled for the host."""
    import tempfile
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.cpp"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write(_PROGRAM % HEADER)
        subprocess.run([cxx, "-std=c++17", "-O0", "-x", "c++", src, "-o", exe], check=True)
        text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    blocks, others, cur = {}, {}, None
    for line in text.splitlines():
        w = line.split()
        if w[0] == "block":
            f = dict(zip("NT H U C KQ RQ RR KEEP ok".split(), map(int, w[1:])))
            cur = blocks[f["C"]] = (f, {})
        elif w[0] == "lane":
            cur[1][int(w[1])] = (int(w[2]), [int(v) for v in w[3:]])
        else:
            others[(int(w[1]), int(w[2]))] = int(w[3])
    return blocks, others


def test_only_h256_u64_takes_the_block_layout():
    blocks, others = _enumerated()
    assert sorted(blocks) == [2, 4]
    assert set(others.values()) == {0} and len(others) == 13


@pytest.mark.parametrize("C", [2, 4])
def test_every_weight_and_every_sum_belongs_to_exactly_one_lane(C):
    f, lanes = _enumerated()[0][C]
    assert f["ok"] == 1 and (f["NT"], f["H"], f["U"], f["C"]) == (NT, H, U, C)
    KQ, RQ, RR, KEEP = f["KQ"], f["RQ"], f["RR"], f["KEEP"]
    assert KQ * RR * NT == 4 * U * H and RQ * H == NT * KQ and RQ <= 64 and RQ & (RQ - 1) == 0 and 64 % RQ == 0
    assert KEEP * NT == C * H and sorted(lanes) == list(range(RQ))
    owners = np.zeros((4 * U, H), dtype=np.int64)
    sums = np.zeros((H, C), dtype=np.int64)
    for tid in range(NT):
        kb, rq = divmod(tid, RQ)
        first, rws = lanes[rq]
        assert len(rws) == RR
        for q in range(KQ):
            owners[rws, KQ * kb + q] += 1
        for v in range(KEEP):
            q, c = divmod(first + v, C)
            assert q == first // C, "a lane's sums are columns c, c + 1, ... of one k"
            sums[KQ * kb + q, c] += 1
        # rows 2 p and 2 p + 1 of a pair side by side: one read of 2 C floats
        assert all(rws[j + 1] == rws[j] + 1 and rws[j] % 2 == 0 for j in range(0, RR, 2))
        # the RQ lanes of a read: adjacent 8 C-byte chunks, no two on one bank
        assert [lanes[r][1][0] for r in range(RQ)] == [2 * r for r in range(RQ)]
    assert (owners == 1).all() and (sums == 1).all()


def test_rows_and_tree_do_not_depend_on_the_columns():
    b = _enumerated()[0]
    assert {rq: v[1] for rq, v in b[2][1].items()} == {rq: v[1] for rq, v in b[4][1].items()}
    assert b[2][0]["RQ"] == b[4][0]["RQ"] and b[2][0]["KQ"] == b[4][0]["KQ"]


@pytest.mark.parametrize("C", [2, 4])
def test_halving_leaves_each_lane_the_sums_the_header_names(C):
    """The kernel's rounds in numpy, float32, one group of RQ lanes: after them lane rq holds, at [0, KEEP), the sums
    kept_first(rq) + v over all lanes, added as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7))."""
    f, lanes = _enumerated()[0][C]
    KQ, RQ, KEEP = f["KQ"], f["RQ"], f["KEEP"]
    rs = np.random.RandomState(C)
    part = rs.standard_normal((RQ, KQ * C)).astype(np.float32)
    acc, n, m = part.copy(), KQ * C, 1
    while m < RQ:
        n //= 2
        new = acc.copy()
        for rq in range(RQ):
            up = bool(rq & m)
            for a in range(n):
                send_of_partner = acc[rq ^ m][a + n] if up else acc[rq ^ m][a]      # the partner is the other half
                keep = acc[rq][a + n] if up else acc[rq][a]
                new[rq][a] = np.float32(keep + send_of_partner)
        acc, m = new, 2 * m
    assert n == KEEP
    tree = lambda s: np.float32(np.float32(np.float32(s[0] + s[1]) + np.float32(s[2] + s[3]))
                                + np.float32(np.float32(s[4] + s[5]) + np.float32(s[6] + s[7])))
    assert RQ == 8
    for rq in range(RQ):
        for v in range(KEEP):
            a = lanes[rq][0] + v
            assert acc[rq][v] == tree(part[:, a]), (rq, v)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_cus = rows._cus
_stopped = []


@pytest.fixture(autouse=True)
def _nothing_after_a_bad_status():
    if _stopped:
        pytest.fail("not run: an earlier launch of this module ended with %s" % (_stopped[0],))


def _finish(rc, status, what):
    if rc != 0:
        _stopped.append((what, "rc", rc))
    _lib.check(rc, what)
    torch.cuda.synchronize()
    word = int(status.item())
    if word != 0:
        _stopped.append((what, "status", word))
    assert word == 0, (what, word)


def _batch(inst, dev):
    n = insts.lstm_batch(inst, _cus(dev))
    insts._check_inst(inst, n, dev)
    assert n % inst[2] == 1, "a ragged last group"
    return n


def _lens(lens, dev):
    return None if lens is None else torch.tensor(lens, dtype=torch.int32, device=dev)


def _scratch(wsb, dev):
    assert wsb > 0
    return torch.empty(wsb, dtype=torch.uint8, device=dev), torch.zeros(1, dtype=torch.int32, device=dev)


def _forward(gx, whh, lens, rev):
    """The saving forward: tk_lstm_forward_dev (lens None) or tk_lstm_forward_varlen_save_dev -> gates, cell."""
    T, N, _ = gx.shape
    dev, cus, P = gx.device, _cus(gx.device), _lib.ptr
    y, gates, cell = (torch.full(s, float("nan"), device=dev) for s in ((T, N, H), (T, N, 4 * H), (T, N, H)))
    if lens is None:
        L = _lib.lib()
        wsb = L.tk_lstm_workspace_bytes(N, H, cus)
        ws, status = _scratch(wsb, dev)
        rc = L.tk_lstm_forward_dev(P(gx), P(whh), T, N, H, rev, cus, P(y), P(gates), P(cell), P(ws), wsb, P(status),
                                   _lib.stream_ptr())
    else:
        V = _lib.varlen_train_lib()
        wsb = V.tk_rnn_varlen_train_workspace_bytes(_lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"], N, H, cus)
        ws, status = _scratch(wsb, dev)
        rc = V.tk_lstm_forward_varlen_save_dev(P(gx), P(whh), P(_lens(lens, dev)), T, N, H, rev, cus, P(y), P(gates),
                                               P(cell), P(ws), wsb, P(status), _lib.stream_ptr())
    _finish(rc, status, "lstm forward")
    return gates, cell


def _backward(build, whh, gates, cell, dy, lens, rev):
    """The backward of one build into a guarded, sentinel-filled dgates: "plain" (tk_lstm_backward_dev), "lab" (the same
    entry of the lab library), "varlen" (tk_lstm_backward_varlen_dev; lens None: lengths = NULL) or "wide"
    (tk_lstm_backward_wide_dev).  Asserts the bounds, every element stored and finite."""
    T, N, _ = dy.shape
    dev, cus, P = dy.device, _cus(dy.device), _lib.ptr
    kind = _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"]
    flat, dg = rows._guarded((T, N, 4 * H), dev, 0)
    if build in ("plain", "lab"):
        assert lens is None
        L = _lib.use_lab(build == "lab")
        try:
            if build == "lab":
                L.tk_lab_lstm_units(0)
            wsb = L.tk_lstm_workspace_bytes(N, H, cus)
            ws, status = _scratch(wsb, dev)
            rc = L.tk_lstm_backward_dev(P(whh), P(gates), P(cell), P(dy), T, N, H, rev, cus, P(dg), P(ws), wsb,
                                        P(status), _lib.stream_ptr())
        finally:
            _lib.use_lab(False)
    else:
        V = _lib.varlen_train_lib() if build == "varlen" else _lib.rnn_wide_lib()
        wsb = (V.tk_rnn_varlen_train_workspace_bytes if build == "varlen" else V.tk_rnn_wide_workspace_bytes)(
            kind, N, H, cus)
        ws, status = _scratch(wsb, dev)
        fn = V.tk_lstm_backward_varlen_dev if build == "varlen" else V.tk_lstm_backward_wide_dev
        rc = fn(P(whh), P(gates), P(cell), P(dy), P(_lens(lens, dev)), T, N, H, rev, cus, P(dg), P(ws), wsb, P(status),
                _lib.stream_ptr())
    _finish(rc, status, "lstm backward (%s)" % build)
    assert rows._guards_intact(flat, 0, dg.numel()), "dgates: a store outside the tensor"
    unwritten = int((dg == rows.SENTINEL).sum().item())
    assert unwritten == 0, ("dgates: elements not stored", unwritten)
    assert bool(torch.isfinite(dg).all())
    return dg


@functools.lru_cache(maxsize=None)
def _case(N, T):
    """gx, a random dense W_hh and dy on the host (seeded by the shape)."""
    g = torch.Generator().manual_seed(35000 + 10 * N + T)
    gx = torch.randn(T, N, 4 * H, generator=g)
    whh = torch.randn(4 * H, H, generator=g) / H ** 0.5
    dy = torch.randn(T, N, H, generator=g) / (T * N) ** 0.5
    assert float((whh == 0).sum()) == 0
    return gx, whh, dy


def _dgates64(gx, whh, dy, lens, rev):
    """d (y * dy).sum() / d gx of the float64 recurrence (masked where lens is given), by autograd."""
    T, N, _ = gx.shape
    g64 = gx.double().requires_grad_(True)
    eye, zero = torch.eye(4 * H, dtype=torch.float64), torch.zeros(4 * H, dtype=torch.float64)
    if lens is None:
        y = rows._float64_lstm(g64, eye, whh.double(), zero, rev)[0]
    else:
        y = insts._masked_lstm(g64, eye, whh.double(), zero, lens, rev)
    (y * dy.double()).sum().backward()
    return g64.grad.detach()


@functools.lru_cache(maxsize=None)
def _reference(N, T, rev, masked):
    gx, whh, dy = _case(N, T)
    return _dgates64(gx, whh, dy, insts.lengths_for(N, T) if masked else None, rev)


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", [3, 7])
@pytest.mark.parametrize("inst", INSTS, ids=_ids)
def test_dgates_match_float64_inside_miopens_bound(gpu_device, inst, T, rev, masked):
    dev, n = gpu_device, _batch(inst, gpu_device)
    gx, whh, dy = (t.to(dev) for t in _case(n, T))
    lens = insts.lengths_for(n, T) if masked else None
    gates, cell = _forward(gx, whh, lens, rev)
    dg = _backward("varlen" if masked else "plain", whh, gates, cell, dy, lens, rev)
    ref = _reference(n, T, rev, masked)
    assert ref.abs().max().item() > 0
    if masked:
        beyond = torch.arange(T)[:, None] >= torch.tensor(lens)[None, :]
        assert int(beyond.sum()) > 0 and bool((dg.cpu()[beyond] == 0).all()), "rows at and beyond the length are 0"
    e = rows._rel(dg, ref)
    e_mio = rows._rel(insts._miopen_dgates(gx, whh, dy, rev), _reference(n, T, rev, False))
    print("lstm bwd layout %s N %d T %d rev %d %s: error %.3e, MIOpen's %.3e, ratio %.3f"
          % (_ids(inst), n, T, rev, "lengths" if masked else "full", e, e_mio, e / insts._allowed(e_mio)))
    assert e <= insts._allowed(e_mio), (inst, n, T, rev, masked, e, e_mio)


def _placement_units():
    """One unit per workgroup member m (units [64 m, 64 m + 64)) and lane residue rq = (unit / 2) % 8 of the row
    partition, both parities and all four runs of 16 units among them."""
    units = [64 * m + 16 * ((rq + m) % 4) + 2 * rq + ((m + rq) & 1) for m in range(H // U) for rq in range(8)]
    assert len(set(units)) == 32 and {(u // U, (u % U // 2) % 8) for u in units} == {(m, r) for m in range(4) for r in range(8)}
    return units


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", INSTS, ids=_ids)
def test_one_unit_of_dy_reaches_every_k_of_the_next_step(gpu_device, inst, rev):
    dev, n, T = gpu_device, _batch(inst, gpu_device), 3
    gx, whh, _ = _case(n, T)
    units = _placement_units()
    t0 = 0 if rev else T - 1                     # the recurrence's first backward step
    t1 = 1 if rev else T - 2                     # ... and its next
    gates, cell = _forward(gx.to(dev), whh.to(dev), None, rev)
    for first in range(0, len(units), n):
        dy = torch.zeros(T, n, H)
        cols = list(range(min(n, len(units) - first)))
        for c in cols:
            dy[t0, c, units[first + c]] = 1.0 + 0.25 * c
        dg = _backward("plain", whh.to(dev), gates, cell, dy.to(dev), None, rev).cpu().double()
        ref = _dgates64(gx, whh, dy, None, rev)
        top = ref[t1].abs().max().item()
        assert top > 1e-4
        err = (dg[t1] - ref[t1]).abs().max().item() / top
        print("lstm bwd layout %s rev %d units %s: next step's error %.3e of its largest entry"
              % (_ids(inst), rev, units[first:first + len(cols)], err))
        assert err <= 1e-6, (inst, rev, first, err)
        assert bool((dg[:, len(cols):] == 0).all()), "a column without dy has no gradient"


@pytest.mark.gpu
@pytest.mark.parametrize("masked", [False, True], ids=["full", "lengths"])
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", INSTS, ids=_ids)
def test_two_calls_give_the_same_bits(gpu_device, inst, rev, masked):
    dev, n, T = gpu_device, _batch(inst, gpu_device), 7
    gx, whh, dy = (t.to(dev) for t in _case(n, T))
    lens = insts.lengths_for(n, T) if masked else None
    gates, cell = _forward(gx, whh, lens, rev)
    build = "varlen" if masked else "plain"
    assert torch.equal(_backward(build, whh, gates, cell, dy, lens, rev), _backward(build, whh, gates, cell, dy, lens, rev))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
def test_a_column_has_the_same_bits_at_2_and_at_4_columns_per_workgroup(gpu_device, rev):
    dev, T = gpu_device, 7
    n4, n2 = _batch((256, 64, 4), dev), _batch((256, 64, 2), dev)
    gx, whh, dy = (t.to(dev) for t in _case(n4, T))
    gates, cell = _forward(gx, whh, None, rev)
    wide = _backward("plain", whh, gates, cell, dy, None, rev)
    for first in (0, 1, n4 - n2):                # every column position of both, and the ragged last group's column
        sl = slice(first, first + n2)
        part = _backward("plain", whh, gates[:, sl].contiguous(), cell[:, sl].contiguous(), dy[:, sl].contiguous(),
                         None, rev)
        assert torch.equal(part, wide[:, sl]), (rev, first, (part - wide[:, sl]).abs().max().item())


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", INSTS, ids=_ids)
def test_every_build_and_lengths_form_gives_the_plain_pairs_bits(gpu_device, inst, rev):
    dev, n, T = gpu_device, _batch(inst, gpu_device), 7
    gx, whh, dy = (t.to(dev) for t in _case(n, T))
    gates, cell = _forward(gx, whh, None, rev)
    want = _backward("plain", whh, gates, cell, dy, None, rev)
    for build, lens in (("lab", None), ("varlen", None), ("varlen", [T] * n), ("wide", None), ("wide", [T] * n)):
        got = _backward(build, whh, gates, cell, dy, lens, rev)
        assert torch.equal(got, want), (inst, rev, build, lens is None, (got - want).abs().max().item())
