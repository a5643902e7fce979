"""The lane layout of the LSTM forward's step at H 256, U 64 (csrc/lstm_fwd_layout.h; lstm_fwd_lanes_body in
csrc/lstm_kernels.hip): h in LDS as 16-byte chunks of a lane's rows, the 8 partial sums of a (gate, column) met by
recursive halving through DPP, one gate's activation per lane, the cell update in the lane of gate i.  The kernel
takes it at (256, 64, 2); (256, 64, 4) measured slower on it and keeps the plain body, so its GPU cases below run
that body: the same checks, and the cases across C compare the two bodies' bits.

CPU: the header compiled for the host and enumerated -- the h image a bijection, every read of a lane one aligned
16-byte chunk of its own rows, every weight in exactly one lane, every (gate, column) of a unit left in exactly one of
its 8 lanes, and the halving, run lane by lane in numpy, leaving the sums the header says in the tree it states, the
same at 2 and at 4 columns.

GPU, at the C ABI, both instantiations ((256, 64, 2) at N = 15, (256, 64, 4) at 8 (CUs // 16) + 1 columns: ragged last
groups), T in {1, 2, 3, 7} (no poll and the store behind the loop; the first poll; the staging block's first reuse;
both parities several times), both directions.  This change reorders no sum, so every check is on bits:
  * y, c and the four gate slabs equal those of the 32-unit kernels ((256, 32, 4 / 8), forced in the lab build), which
    have the same 8 lanes per unit, the same k per lane and the same butterfly, and which this layout does not touch;
    also on inputs whose pre-activations lie at 0, inside +-0.5, at a few units and beyond +-90 (both branches of tanhf,
    expf's overflow and underflow in sigmoidf), where the outputs must also be finite;
  * a column's bits are the same at 2 and at 4 columns per workgroup; two calls give the same bits;
  * the release, lab, variable-length training and wide builds agree, with lengths NULL and with lengths (some columns
    shorter than T, some of length 0), the y-only launches give the same y, and a step at or beyond a column's length
    leaves y = c = 0 and zeros in the saved gates;
  * every output sits one float off 16-byte alignment between guard bands over a sentinel: every element is stored,
    nothing outside is (a store for a missing column of the ragged group would land there), and the workspace, exactly
    the size asked, lies between guards of its own.

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
STEPS = [1, 2, 3, 7]
HEADER = os.path.join(_lib.CSRC, "lstm_fwd_layout.h")
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
        const tk::LstmFwdLanes f(c[0], c[1], c[2], c[3]);
        std::printf("layout %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d %%d\n", f.NT, f.H, f.U, f.C, f.KP, f.KS, f.PR, f.CK,
                    (int)f.ok(), f.gate_lane_xor(1), f.gate_lane_xor(2), f.gate_lane_xor(3));
        for (int kp = 0; kp < f.KP; ++kp) {
            std::printf("lane %%d %%d %%d %%d %%d", kp, f.kept_first(kp), f.gate(kp), f.col(kp, 0), (int)f.cell_lane(kp));
            for (int i = 0; i < f.KS; ++i) std::printf(" %%d", f.k(kp, i));
            std::printf("\nchunks %%d", kp);
            for (int j = 0; j < f.KS / f.PR; ++j) std::printf(" %%d", f.chunk(kp, j));
            std::printf("\n");
        }
        std::printf("hs");
        for (int k = 0; k < f.H; ++k)
            for (int cc = 0; cc < f.C; ++cc) std::printf(" %%d", f.hs_index(k, cc));
        std::printf("\nflat");
        for (int g = 0; g < 4; ++g)
            for (int cc = 0; cc < f.C; ++cc) std::printf(" %%d", f.flat(g, cc));
        std::printf("\n");
    }
    const int others[][2] = {{16, 16}, {32, 16}, {32, 32}, {64, 16}, {64, 32}, {64, 64}, {128, 16}, {128, 32}, {128, 64},
                             {256, 16}, {256, 32}, {192, 48}, {384, 48}, {256, 64}};
    for (auto &o : others)
        for (int c = 2; c <= 16; c *= 2) std::printf("takes %%d %%d %%d %%d\n", o[0], o[1], c, (int)tk::lstm_fwd_lanes(o[0], o[1], c));
    return 0;
}
"""


@functools.lru_cache(maxsize=None)
def _enumerated():
    """{C: {fields, lanes {kp: (kept_first, gate, col0, cell_lane, [k])}, chunks {kp: [float]}, hs (H, C), flat (4, C)}}
    and {(H, U): takes the layout} from the header, compiled for the host."""
    import tempfile
    cxx = next((c for c in ("c++", "g++", "clang++", "/opt/rocm/bin/hipcc") if shutil.which(c)), None)
    assert cxx, "no host C++ compiler"
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "layout.cpp"), os.path.join(d, "layout")
        with open(src, "w") as fh:
            fh.write(_PROGRAM % HEADER)
        subprocess.run([cxx, "-std=c++17", "-O0", "-x", "c++", src, "-o", exe], check=True)
        text = subprocess.run([exe], check=True, capture_output=True, text=True).stdout
    layouts, takes, cur = {}, {}, None
    for line in text.splitlines():
        w = line.split()
        v = [int(x) for x in w[1:]]
        if w[0] == "layout":
            f = dict(zip("NT H U C KP KS PR CK ok x1 x2 x3".split(), v))
            cur = layouts[f["C"]] = {"f": f, "lanes": {}, "chunks": {}}
        elif w[0] == "lane":
            cur["lanes"][v[0]] = (v[1], v[2], v[3], v[4], v[5:])
        elif w[0] == "chunks":
            cur["chunks"][v[0]] = v[1:]
        elif w[0] == "hs":
            cur["hs"] = np.array(v).reshape(cur["f"]["H"], cur["f"]["C"])
        elif w[0] == "flat":
            cur["flat"] = np.array(v).reshape(4, cur["f"]["C"])
        else:
            takes[(v[0], v[1], v[2])] = v[3]
    return layouts, takes


def test_only_256_64_2_takes_the_lane_layout():
    """(256, 64, 4) does not: its arithmetic is enumerated below all the same (the tree must not depend on C), and its
    GPU cases run the plain body, whose bits the cases across C compare with the lane layout's."""
    layouts, takes = _enumerated()
    assert sorted(layouts) == [2, 4] and len(takes) == 14 * 4
    assert {k for k, v in takes.items() if v} == {(256, 64, 2)}


@pytest.mark.parametrize("C", [2, 4])
def test_h_image_is_a_bijection_of_aligned_16_byte_chunks_of_a_lanes_rows(C):
    L = _enumerated()[0][C]
    f = L["f"]
    assert f["ok"] == 1 and (f["NT"], f["H"], f["U"], f["C"]) == (NT, H, U, C)
    KP, KS, PR = f["KP"], f["KS"], f["PR"]
    assert KP == 8 and KS * KP == H and PR * C == 4, "a read is 16 bytes: 4 / C whole rows"
    hs = L["hs"]
    assert sorted(hs.ravel().tolist()) == list(range(H * C)), "every float of the image holds exactly one (k, c)"
    for kp in range(KP):
        ks, chunks = L["lanes"][kp][4], L["chunks"][kp]
        assert ks == [i * KP + kp for i in range(KS)] and len(chunks) == KS // PR
        for j, first in enumerate(chunks):
            assert first % 4 == 0, "16-byte aligned"
            want = [hs[ks[PR * j + e], c] for e in range(PR) for c in range(C)]
            assert want == list(range(first, first + 4)), "rows PR j ... of the lane, C floats each, in one chunk"
            # the 8 lanes of a read: 8 adjacent chunks (the other lanes of the wave read the same 8)
            assert first == L["chunks"][0][j] + 4 * kp
    if C == 4:
        assert (hs == np.arange(H * C).reshape(H, C)).all(), "at 4 columns a row is 16 bytes: the plain [k][c] image"


@pytest.mark.parametrize("C", [2, 4])
def test_every_weight_and_every_gate_of_a_column_belongs_to_exactly_one_lane(C):
    L = _enumerated()[0][C]
    f, flat = L["f"], L["flat"]
    KP, KS, CK = f["KP"], f["KS"], f["CK"]
    assert CK * KP == 4 * C and sorted(flat.ravel().tolist()) == list(range(4 * C))
    owners = np.zeros((4 * U, H), dtype=np.int64)
    kept = np.zeros((U, 4, C), dtype=np.int64)
    for tid in range(NT):
        u, kp = divmod(tid, KP)
        first, gate, col0, cell_lane, ks = L["lanes"][kp]
        for g in range(4):
            owners[g * U + u, ks] += 1
        for v in range(CK):
            (g,), (c,) = np.nonzero(flat == first + v)
            assert (g, c) == (gate, col0 + v), "the lane's sums: one gate, columns col, col + 1, ..."
            kept[u, g, c] += 1
        assert cell_lane == (gate == 0)
    assert (owners == 1).all() and (kept == 1).all()
    # the other three gates of the cell lane's columns, as an xor of kp: f, g, o
    assert (f["x1"], f["x2"], f["x3"]) == (4, 2, 6)
    for kp in range(KP):
        first, gate, col0, cell_lane, _ = L["lanes"][kp]
        if cell_lane:
            for g, x in ((1, 4), (2, 2), (3, 6)):
                assert L["lanes"][kp ^ x][1:3] == (g, col0)


def test_weights_gates_and_tree_do_not_depend_on_the_columns():
    b = _enumerated()[0]
    assert {kp: (v[1], v[3], v[4]) for kp, v in b[2]["lanes"].items()} == \
           {kp: (v[1], v[3], v[4]) for kp, v in b[4]["lanes"].items()}
    assert b[2]["f"]["KP"] == b[4]["f"]["KP"] and b[2]["f"]["KS"] == b[4]["f"]["KS"]


@pytest.mark.parametrize("C", [2, 4])
def test_halving_leaves_each_lane_the_sums_the_header_names(C):
    """halve_rounds in numpy, float32, the 8 lanes of one unit: after it lane kp holds, at [0, CK), the sums
    kept_first(kp) + v over all lanes, each added as ((0 + 1) + (2 + 3)) + ((4 + 5) + (6 + 7)) -- the tree of the plain
    body's xor shuffles, at either C."""
    L = _enumerated()[0][C]
    KP, CK = L["f"]["KP"], L["f"]["CK"]
    rs = np.random.RandomState(C)
    part = rs.standard_normal((KP, 4 * C)).astype(np.float32)
    acc, n, m = part.copy(), 4 * C, 1
    while m < KP:
        n //= 2
        new = acc.copy()
        for kp in range(KP):
            up = bool(kp & m)
            for a in range(n):
                sent = acc[kp ^ m][a + n] if up else acc[kp ^ m][a]      # the partner sends the half it does not keep
                keep = acc[kp][a + n] if up else acc[kp][a]
                new[kp][a] = np.float32(keep + sent)
        acc, m = new, 2 * m
    assert n == CK and KP == 8
    tree = lambda s: np.float32(np.float32(np.float32(s[0] + s[1]) + np.float32(s[2] + s[3]))
                                + np.float32(np.float32(s[4] + s[5]) + np.float32(s[6] + s[7])))
    for kp in range(KP):
        for v in range(CK):
            assert acc[kp][v] == tree(part[:, L["lanes"][kp][0] + v]), (kp, v)


# ---------------------------------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------------------------------
_cus = rows._cus
_stopped = []
WS_GUARD = 4096                  # bytes in front of and behind the workspace
KIND = _lib.VARLEN_DEFINES["TK_RNN_KIND_LSTM"]


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


def _run(build, gx, whh, lens, rev, units=0):
    """One forward of `build` into sentinel-filled outputs one float off 16-byte alignment, between guards, on a
    workspace of exactly the size asked, between guards too.  "plain": tk_lstm_forward_dev; "lab": the same entry of the
    lab library at `units` units per workgroup (0: the release rule); "vltrain": tk_lstm_forward_varlen_save_dev;
    "wide": tk_lstm_forward_wide_dev; "varlen" and "wide_y": the launches that save nothing (gates, cell: None).
    Asserts the guards, every element stored and finite; returns y, gates, cell."""
    T, N, _ = gx.shape
    dev, cus, P = gx.device, _cus(gx.device), _lib.ptr
    saving = build not in ("varlen", "wide_y")
    shapes = ((T, N, H), (T, N, 4 * H), (T, N, H)) if saving else ((T, N, H),)
    bufs = [rows._guarded(s, dev, 1) for s in shapes]
    y = bufs[0][1]
    gates, cell = (bufs[1][1], bufs[2][1]) if saving else (None, None)
    assert all(b.data_ptr() % 16 == 4 for _, b in bufs)
    status = torch.zeros(1, dtype=torch.int32, device=dev)

    def scratch(wsb):
        assert wsb > 0 and wsb % 16 == 0
        flat = torch.full((WS_GUARD + wsb + WS_GUARD,), 0xA5, dtype=torch.uint8, device=dev)
        ws = flat[WS_GUARD:WS_GUARD + wsb]
        assert ws.data_ptr() % 16 == 0
        return flat, ws

    if build in ("plain", "lab"):
        assert lens is None
        L = _lib.use_lab(build == "lab")
        try:
            if build == "lab":
                L.tk_lab_lstm_units(units)
            wsb = L.tk_lstm_workspace_bytes(N, H, cus)
            flat, ws = scratch(wsb)
            rc = L.tk_lstm_forward_dev(P(gx), P(whh), T, N, H, rev, cus, P(y), P(gates), P(cell), P(ws), wsb, P(status),
                                       _lib.stream_ptr())
        finally:
            if build == "lab":
                L.tk_lab_lstm_units(0)
            _lib.use_lab(False)
    elif build == "vltrain":
        V = _lib.varlen_train_lib()
        wsb = V.tk_rnn_varlen_train_workspace_bytes(KIND, N, H, cus)
        flat, ws = scratch(wsb)
        rc = V.tk_lstm_forward_varlen_save_dev(P(gx), P(whh), P(_lens(lens, dev)), T, N, H, rev, cus, P(y), P(gates),
                                               P(cell), P(ws), wsb, P(status), _lib.stream_ptr())
    elif build in ("wide", "wide_y"):
        V = _lib.rnn_wide_lib()
        wsb = V.tk_rnn_wide_workspace_bytes(KIND, N, H, cus)
        flat, ws = scratch(wsb)
        rc = V.tk_lstm_forward_wide_dev(P(gx), P(whh), P(_lens(lens, dev)), T, N, H, rev, cus, P(y), P(gates), P(cell),
                                        P(ws), wsb, P(status), _lib.stream_ptr())
    else:
        assert build == "varlen"
        V = _lib.varlen_lib()
        wsb = V.tk_rnn_varlen_workspace_bytes(KIND, N, H, cus)
        flat, ws = scratch(wsb)
        rc = V.tk_lstm_forward_varlen_dev(P(gx), P(whh), P(_lens(lens, dev)), T, N, H, rev, cus, P(y), P(ws), wsb,
                                          P(status), _lib.stream_ptr())
    _finish(rc, status, "lstm forward (%s)" % build)
    assert bool((flat[:WS_GUARD] == 0xA5).all()) and bool((flat[WS_GUARD + wsb:] == 0xA5).all()), "a store outside the workspace"
    for name, (fl, body) in zip(("y", "gates", "cell"), bufs):
        assert rows._guards_intact(fl, 1, body.numel()), (build, name, "a store outside the tensor")
        unwritten = int((body == rows.SENTINEL).sum().item())
        assert unwritten == 0, (build, name, "elements not stored", unwritten)
        assert bool(torch.isfinite(body).all()), (build, name)
    return y, gates, cell


@functools.lru_cache(maxsize=None)
def _case(N, T, extreme=False):
    """gx and a random dense W_hh on the host (seeded by the shape).  extreme: the pre-activations gx + W_hh h (|h| < 1,
    so the second term is a few tenths) lie at 0, inside +-0.5, at a few units and beyond +-90, a quarter each."""
    g = torch.Generator().manual_seed(36000 + 10 * N + T + 5 * extreme)
    gx = torch.randn(T, N, 4 * H, generator=g)
    whh = torch.randn(4 * H, H, generator=g) / H ** 0.5
    if extreme:
        kind = torch.randint(0, 4, gx.shape, generator=g)
        sign = torch.randint(0, 2, gx.shape, generator=g).float() * 2 - 1
        unit = torch.rand(gx.shape, generator=g)
        gx = torch.where(kind == 0, torch.zeros_like(gx),
                         torch.where(kind == 1, unit - 0.5, torch.where(kind == 2, 3 * gx, sign * (90 + 20 * unit))))
        whh = whh * 0.25
        assert all(int((kind == q).sum()) > 0 for q in range(4))
    return gx, whh


def _same(got, want, what):
    for name, a, b in zip(("y", "gates", "cell"), got, want):
        if a is None or b is None:
            continue
        assert torch.equal(a, b), (what, name, (a - b).abs().max().item(), int((a != b).sum().item()))


def _units32(inst, n, dev):
    """The 32-unit plan of the lab build at this batch: (256, 32, 2 C), the same admitted columns."""
    import ctypes
    L = _lib.use_lab(True)
    try:
        L.tk_lab_lstm_units(32)
        out = (ctypes.c_size_t * 8)()
        assert L.tk_lab_lstm_geometry(n, H, _cus(dev), out)
        assert (int(out[2]), int(out[3])) == (32, 2 * inst[2]), (inst, n, list(out))
    finally:
        L.tk_lab_lstm_units(0)
        _lib.use_lab(False)


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("inst", INSTS, ids=_ids)
def test_bits_are_those_of_the_32_unit_kernels(gpu_device, inst, T, rev):
    dev, n = gpu_device, _batch(inst, gpu_device)
    _units32(inst, n, dev)
    gx, whh = (t.to(dev) for t in _case(n, T))
    _same(_run("plain", gx, whh, None, rev), _run("lab", gx, whh, None, rev, units=32), (inst, T, rev))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", INSTS, ids=_ids)
def test_every_branch_of_the_activation_lanes_gives_the_32_unit_kernels_bits(gpu_device, inst, rev):
    dev, n, T = gpu_device, _batch(inst, gpu_device), 3
    gx, whh = (t.to(dev) for t in _case(n, T, True))
    got = _run("plain", gx, whh, None, rev)                     # (finite: asserted there)
    _same(got, _run("lab", gx, whh, None, rev, units=32), (inst, rev))
    gates = got[1].cpu()
    sig = torch.cat([gates[..., :2 * H], gates[..., 3 * H:]], -1)
    assert float(sig.min()) == 0.0 and float(sig.max()) == 1.0, "sigmoidf at both ends of expf's range"
    assert float(gates[..., 2 * H:3 * H].min()) == -1.0 and float(gates[..., 2 * H:3 * H].max()) == 1.0
    assert int((gates[..., 2 * H:3 * H].abs() < 0.4).sum()) > 0, "tanhf's branch for small arguments"


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
def test_a_column_has_the_same_bits_at_2_and_at_4_columns_per_workgroup(gpu_device, rev):
    dev, T = gpu_device, 7
    n4, n2 = _batch((256, 64, 4), dev), _batch((256, 64, 2), dev)
    gx, whh = (t.to(dev) for t in _case(n4, T))
    wide = _run("plain", gx, whh, None, rev)
    part = _run("plain", gx[:, :n2].contiguous(), whh, None, rev)
    _same(part, [t[:, :n2] for t in wide], rev)


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", INSTS, ids=_ids)
def test_two_calls_give_the_same_bits(gpu_device, inst, rev):
    dev, n, T = gpu_device, _batch(inst, gpu_device), 7
    gx, whh = (t.to(dev) for t in _case(n, T))
    _same(_run("plain", gx, whh, None, rev), _run("plain", gx, whh, None, rev), (inst, rev))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("inst", INSTS, ids=_ids)
def test_every_build_gives_the_same_bits_without_lengths(gpu_device, inst, rev):
    dev, n, T = gpu_device, _batch(inst, gpu_device), 7
    gx, whh = (t.to(dev) for t in _case(n, T))
    want = _run("plain", gx, whh, None, rev)
    for build, lens in (("lab", None), ("vltrain", None), ("vltrain", [T] * n), ("wide", None), ("wide", [T] * n),
                        ("varlen", None), ("varlen", [T] * n), ("wide_y", None)):
        _same(_run(build, gx, whh, lens, rev), want, (inst, rev, build, lens is None))


@pytest.mark.gpu
@pytest.mark.parametrize("rev", [0, 1])
@pytest.mark.parametrize("T", [3, 7])
@pytest.mark.parametrize("inst", INSTS, ids=_ids)
def test_builds_agree_with_lengths_and_masked_steps_are_zero(gpu_device, inst, T, rev):
    dev, n = gpu_device, _batch(inst, gpu_device)
    gx, whh = (t.to(dev) for t in _case(n, T))
    lens = insts.lengths_for(n, T)
    assert 0 in lens and T in lens and any(0 < v < T for v in lens)
    want = _run("vltrain", gx, whh, lens, rev)
    for build in ("wide", "varlen", "wide_y"):
        _same(_run(build, gx, whh, lens, rev), want, (inst, T, rev, build))
    beyond = (torch.arange(T)[:, None] >= torch.tensor(lens)[None, :]).to(dev)
    for name, t in zip(("y", "gates", "cell"), want):
        assert bool((t[beyond] == 0).all()), (name, "a step at or beyond the length is 0")
    if not rev:
        # forward in time a column's steps below its length do not see the mask: they are the unmasked launch's
        full = _run("plain", gx, whh, None, rev)
        for name, a, b in zip(("y", "gates", "cell"), want, full):
            assert torch.equal(a[~beyond], b[~beyond]), name
