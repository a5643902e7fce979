"""Modified-base calls of cat-mod models in the device basecaller: tk_basecall_mod_weights_dev
(include/taiyaki_amd_basecall.h, (f)), `flipflopfings.extract_mod_weights` on device tensors, `Basecaller.call_mods`.

Fixture: tests/golden/mod_weights_small.npz, the genuine reference's `extract_mod_weights` on the seeded cases of
tests/mods_support.py (make_golden_mod_weights.py).  The stitched contract is restated in numpy there
(`stitched_mods`: `stitch_chunks` on paths and weights, the move rule, the column map).

The kernel only copies, so every comparison of modified-base scores is `same_bits`: equal NaN masks and equal float32
bit patterns everywhere else.  No tolerance.

CPU: the restatement against the reference, the ABI, the argument checks.  GPU: the kernel on crafted reads, batch
against single launches, the dense operator on the golden cases, whole `call_mods` runs against the chain of existing
operators."""
import ctypes
import os

import numpy as np
import pytest

from tests import basecall_support as bs
from tests import mods_support as ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BAD_ARG, UNSUPPORTED, CHUNK_PLAN = 1, 2, 256       # TK_ERR_BAD_ARG, TK_ERR_UNSUPPORTED, TK_STATUS_CHUNK_PLAN
ENTRY = "tk_basecall_mod_weights_dev"


# ----------------------------------------------------------------------------------------------------------------------
# CPU
# ----------------------------------------------------------------------------------------------------------------------
def _gold():
    return np.load(ms.GOLDEN)


@pytest.mark.parametrize("case", ms.golden_cases(), ids=lambda c: c[0])
def test_restatement_reproduces_the_reference(case):
    name, can_nmods, T, kind, seed = case
    g = _gold()
    w, path = ms.golden_inputs(can_nmods, T, kind, seed)
    assert np.array_equal(w.view(np.uint32), g[name + "/weights"].view(np.uint32))      # the fixture's inputs
    assert np.array_equal(path, g[name + "/path"])
    want = g[name + "/mods"]
    assert want.dtype == np.float32 and np.isnan(want[0]).all()
    assert ms.same_bits(ms.moves_to_mods(w, path, can_nmods), want[1:])
    # as a read of one chunk through the stitched form: all rows kept
    got = ms.stitched_mods(path[:, None], w[:, None], np.array([0]), np.array([5 * T]), 5, can_nmods)
    assert ms.same_bits(got, want[1:])
    assert len(want) - 1 == {"nomove": 0, "allmove": T}.get(kind, len(want) - 1)


def _exported(path):
    import subprocess
    out = subprocess.run(["nm", "-D", "--defined-only", path], capture_output=True, text=True, check=True).stdout
    return {ln.split()[2] for ln in out.splitlines() if len(ln.split()) == 3 and ln.split()[1] in "TDBW"}


def test_entry_point_is_declared_exported_and_bound():
    from taiyaki_amd import _lib
    _lib.build()
    hdr = open(os.path.join(ROOT, "include", "taiyaki_amd_basecall.h")).read()
    assert "int %s(" % ENTRY in hdr and "flipflopfings.py:100-143" in hdr
    assert ENTRY in _exported(os.path.join(_lib.CSRC, _lib.BASECALL_LIBNAME))
    res, args = _lib.BASECALL_SIGNATURES[ENTRY]
    assert res is ctypes.c_int and len(args) == 17
    assert _lib.BASECALL_DEFINES["TK_BASECALL_MAX_NMOD"] >= 2
    # the flip-flop library gained nothing: its exports are still its header's table, to the symbol
    flipflop = _exported(_lib.LIBPATH)
    assert flipflop == set(_lib.SIGNATURES) and not any("mod_weights" in s for s in flipflop)
    assert _lib.basecall_lib().tk_basecall_version() == b"taiyaki_amd basecall gfx950 r2"


def test_construction_errors_come_before_the_device_check():
    """CPU models: each of these raises ValueError, not the RuntimeError of a model that is not on a GPU."""
    from taiyaki_amd import basecall, layers, models
    plain = models.mLstm_flipflop(size=16)
    catmod = models.mLstm_cat_mod_flipflop(size=16)
    nomod = models.mLstm_cat_mod_flipflop(size=16, can_nmods=(0, 0, 0, 0))
    assert layers.is_cat_mod_model(catmod) and not layers.is_cat_mod_model(plain)
    assert layers.is_cat_mod_model(models.mGru_cat_mod_flipflop(size=16))
    with pytest.raises(ValueError, match="GlobalNormFlipFlopCatMod"):
        basecall.Basecaller(plain, stride=5, mod_output=True)
    with pytest.raises(ValueError, match="without a modification"):
        basecall.Basecaller(nomod, stride=5, mod_output=True)
    with pytest.raises(ValueError, match="beam"):
        basecall.Basecaller(catmod, stride=5, mod_output=True, beam=(5, True))
    with pytest.raises(RuntimeError, match="no CPU fallback"):          # and then the device check, as before
        basecall.Basecaller(catmod, stride=5, mod_output=True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        basecall.Basecaller(catmod, stride=5)


def test_dense_operator_has_no_cpu_fallback():
    import torch
    from taiyaki_amd import flipflopfings
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        flipflopfings.extract_mod_weights(torch.zeros(5, 6), torch.zeros(6, dtype=torch.int64), (1, 1, 0, 0))


@pytest.mark.parametrize("can_nmods, want", [((0, 0, 0, 0), BAD_ARG), (None, BAD_ARG), ((33, 0, 0, 0), UNSUPPORTED),
                                             ((16, 16, 0, 1), UNSUPPORTED), ((1, -1, 1, 0), BAD_ARG)])
def test_argument_checks_need_no_device(can_nmods, want):
    """Returned before anything is launched: the pointers are host memory that is never read."""
    from taiyaki_amd import _lib
    L = _lib.basecall_lib()
    assert _lib.BASECALL_DEFINES["TK_BASECALL_MAX_NMOD"] == 32
    assert (_lib.DEFINES["TK_ERR_BAD_ARG"], _lib.DEFINES["TK_ERR_UNSUPPORTED"]) == (BAD_ARG, UNSUPPORTED)
    assert _lib.BASECALL_DEFINES["TK_STATUS_CHUNK_PLAN"] == CHUNK_PLAN
    mem = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(mem))
    cm = (ctypes.c_int * 4)(*can_nmods) if can_nmods is not None else None
    assert L.tk_basecall_mod_weights_dev(p, p, 10, 1, p, p, p, None, 1, 5, 4, cm, p, p, p, None, None) == want


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the kernel on crafted reads.  Every launch happens once per check; nothing loops on a failing launch.
# ----------------------------------------------------------------------------------------------------------------------
NBLK, STRIDE, OVERLAP = 100, 5, 100                 # blocks per chunk, samples per block, samples of overlap
CHUNK = NBLK * STRIDE
SENTINEL = np.uint32(0xDEADBEEF)


def _p(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _geometry(nch, ragged):
    from taiyaki_amd import basecall_helpers
    if nch == 0:
        return np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    siglen = CHUNK + (nch - 1) * (CHUNK - OVERLAP) - (ragged if nch > 1 else 0)
    starts, ends = basecall_helpers.chunk_bounds(siglen, CHUNK, OVERLAP)
    assert len(starts) == nch
    return starts.astype(np.int64), ends.astype(np.int64)


def _scatter(stitched, starts, ends, seed):
    """Per-chunk paths (NBLK + 1, nch) whose stitching is `stitched`; the rows the cuts drop hold other states."""
    nch = len(starts)
    keep = bs.cuts(starts, ends, STRIDE, NBLK + 1)
    assert sum(hi - lo for lo, hi in keep) == len(stitched)
    path = np.random.RandomState(seed).randint(8, size=(NBLK + 1, nch)).astype(np.int64)
    at = 0
    for i, (lo, hi) in enumerate(keep):
        path[lo:hi, i] = stitched[at:at + hi - lo]
        at += hi - lo
    return path, keep


@pytest.fixture(scope="module")
def crafted():
    """Eight reads in one launch: 1, 2, 3 and 5 chunks; one without a move; one refused (NaN scale); one without
    chunks; one more of one chunk behind it.  The read of 5 chunks has more than 256 stitched rows, moves at stitched
    rows 255, 256 and 257, a state change exactly across its first cut and none across its second."""
    spec = [(1, 0, "random"), (2, 37, "random"), (3, 123, "random"), (5, 211, "random"), (1, 0, "nomove"),
            (2, 59, "random"), (0, 0, "random"), (1, 0, "random")]
    reads, paths = [], []
    for r, (nch, ragged, kind) in enumerate(spec):
        starts, ends = _geometry(nch, ragged)
        if nch == 0:
            reads.append(dict(starts=starts, ends=ends, stitched=np.zeros(0, dtype=np.int64), nch=0))
            continue
        nrows = sum(hi - lo for lo, hi in bs.cuts(starts, ends, STRIDE, NBLK + 1))
        stitched = ms.flipflop_path(nrows, 900 + r, kind)
        if nch == 5:
            cut1 = bs.cuts(starts, ends, STRIDE, NBLK + 1)[0]
            c1 = cut1[1] - cut1[0]                                      # first stitched row of chunk 1
            lo2, hi2 = bs.cuts(starts, ends, STRIDE, NBLK + 1)[1]
            c2 = c1 + hi2 - lo2                                         # ... and of chunk 2
            assert nrows > 258 and c2 < 250
            stitched[254:258] = [0, 1, 2, 3]                            # moves at 255, 256, 257
            stitched[c1 - 1:c1 + 1] = [5, 2]                            # a change exactly across the cut
            stitched[c2 - 2:c2 + 2] = [7, 6, 6, 3]                      # no change across this one
        path, _ = _scatter(stitched, starts, ends, 950 + r)
        reads.append(dict(starts=starts, ends=ends, stitched=stitched, nch=nch))
        paths.append(path)
    path = np.concatenate(paths, axis=1)
    rco = np.concatenate([[0], np.cumsum([rd["nch"] for rd in reads])]).astype(np.int64)
    scale = np.ones(len(reads), dtype=np.float32)
    scale[5] = np.nan
    return dict(reads=reads, path=path, rco=rco, scale=scale,
                starts=np.concatenate([rd["starts"] for rd in reads]), ends=np.concatenate([rd["ends"] for rd in reads]))


def _expected(c, r, w, can_nmods):
    """The restatement for read r of the crafted launch (weights w: (NBLK, nchunks, ncat))."""
    lo, hi = int(c["rco"][r]), int(c["rco"][r + 1])
    if hi == lo or np.isnan(c["scale"][r]):
        return np.zeros((0, sum(can_nmods)), dtype=np.float32)
    return ms.stitched_mods(c["path"][:, lo:hi], w[:, lo:hi], c["starts"][lo:hi], c["ends"][lo:hi], STRIDE, can_nmods)


def _launch(dev, path, w, starts, ends, rco, scale, can_nmods, room=None, with_tail=False):
    """One launch -> (mods buffer as uint32 (rows, nmod), out_off, seqlen, status[, the tail's seqlen])"""
    import torch
    from taiyaki_amd import _lib
    L = _lib.basecall_lib()
    nread, nmod, nch = len(rco) - 1, sum(can_nmods), path.shape[1]
    if room is None:
        room = [(NBLK + 1) * int(rco[r + 1] - rco[r]) for r in range(nread)]
    out_off = np.concatenate([[0], np.cumsum(room)]).astype(np.int64)
    t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(dev)  # noqa: E731
    d = dict(path=t(path, np.int64), w=t(w, np.float32), starts=t(starts, np.int64), ends=t(ends, np.int64),
             rco=t(rco, np.int64), scale=t(scale, np.float32), out_off=t(out_off, np.int64))
    rows = int(out_off[-1]) + 4                                         # (four rows nobody owns behind the last read)
    mods = torch.from_numpy(np.full((rows, nmod), SENTINEL, dtype=np.uint32).view(np.int32)).to(dev)
    seqlen = torch.full((nread,), -1, dtype=torch.int32, device=dev)
    status = torch.zeros(1, dtype=torch.int32, device=dev)
    cm = (ctypes.c_int * len(can_nmods))(*can_nmods)
    rc = L.tk_basecall_mod_weights_dev(_p(d["path"]), _p(d["w"]), NBLK, nch, _p(d["starts"]), _p(d["ends"]), _p(d["rco"]),
                                       _p(d["scale"]), nread, STRIDE, len(can_nmods), cm, _p(d["out_off"]), _p(mods),
                                       _p(seqlen), _p(status), None)
    assert rc == 0, rc
    res = [mods.cpu().numpy().view(np.uint32), out_off, seqlen.cpu().numpy(), int(status.item())]
    if with_tail:
        seq = torch.zeros(rows, dtype=torch.uint8, device=dev)
        tail_len = torch.full((nread,), -1, dtype=torch.int32, device=dev)
        rc = L.tk_basecall_call_dev(_p(d["path"]), None, NBLK, nch, _p(d["starts"]), _p(d["ends"]), _p(d["rco"]),
                                    _p(d["scale"]), nread, STRIDE, len(can_nmods), b"ACGT", 1.0, 0.0, _p(d["out_off"]),
                                    _p(seq), None, _p(tail_len), None, None)
        assert rc == 0, rc
        res.append(tail_len.cpu().numpy())
    return res


def _check_reads(buf, out_off, seqlen, want):
    """Read r's rows are `want[r]`, bit for bit; every other word of the buffer still holds the sentinel."""
    untouched = np.ones(buf.shape[0], dtype=bool)
    for r, w in enumerate(want):
        lo = int(out_off[r])
        assert seqlen[r] == len(w), (r, seqlen[r], len(w))
        assert ms.same_bits(buf[lo:lo + len(w)].view(np.float32), w), r
        untouched[lo:lo + len(w)] = False
    assert (buf[untouched] == SENTINEL).all()


@pytest.mark.gpu
@pytest.mark.parametrize("can_nmods", ms.CAN_NMODS)
def test_kernel_matches_the_restatement(gpu_device, crafted, can_nmods):
    c = crafted
    w = ms.weights((NBLK, c["path"].shape[1], 4 + sum(can_nmods)), 77)
    want = [_expected(c, r, w, can_nmods) for r in range(len(c["reads"]))]
    # the crafted moves are where they were meant to be
    st = c["reads"][3]["stitched"]
    assert len(st) > 258 and all(st[k] != st[k - 1] for k in (255, 256, 257))
    assert [len(x) for x in want][4:7] == [0, 0, 0] and min(len(want[r]) for r in (0, 1, 2, 3, 7)) > 10
    buf, out_off, seqlen, status, tail_len = _launch(gpu_device, c["path"], w, c["starts"], c["ends"], c["rco"],
                                                     c["scale"], can_nmods, with_tail=True)
    print("can_nmods", can_nmods, "rows per read", seqlen.tolist())
    assert status == 0
    assert np.array_equal(seqlen, tail_len)                             # what tk_basecall_call_dev writes
    _check_reads(buf, out_off, seqlen, want)
    # every finite output float is an input float
    rows = np.concatenate(want)
    assert np.isin(rows.view(np.uint32)[~np.isnan(rows)], w.view(np.uint32)).all()


@pytest.mark.gpu
def test_kernel_room_one_row_short(gpu_device, crafted):
    c, can_nmods = crafted, (1, 1, 0, 0)
    lo, hi = int(c["rco"][3]), int(c["rco"][4])
    w = ms.weights((NBLK, hi - lo, 6), 78)
    args = (c["path"][:, lo:hi], w, c["starts"][lo:hi], c["ends"][lo:hi], np.array([0, hi - lo]), np.ones(1, np.float32))
    want = ms.stitched_mods(args[0], w, args[2], args[3], STRIDE, can_nmods)
    buf, out_off, seqlen, status = _launch(gpu_device, *args, can_nmods, room=[len(want) - 1])
    assert status == CHUNK_PLAN and seqlen[0] == len(want) - 1
    _check_reads(buf, out_off, seqlen, [want[:-1]])
    buf, out_off, seqlen, status = _launch(gpu_device, *args, can_nmods, room=[len(want)])       # an exact fit
    assert status == 0
    _check_reads(buf, out_off, seqlen, [want])


@pytest.mark.gpu
def test_kernel_batch_equals_single_launches_and_repeats(gpu_device, crafted):
    c, can_nmods = crafted, (2, 0, 1, 0)
    w = ms.weights((NBLK, c["path"].shape[1], 7), 79)
    full = (c["path"], w, c["starts"], c["ends"], c["rco"], c["scale"])
    buf, out_off, seqlen, status = _launch(gpu_device, *full, can_nmods)
    again = _launch(gpu_device, *full, can_nmods)
    assert np.array_equal(buf, again[0]) and np.array_equal(seqlen, again[2])
    for r in range(len(c["reads"])):
        lo, hi = int(c["rco"][r]), int(c["rco"][r + 1])
        if hi == lo:
            continue
        b1, _, n1, s1 = _launch(gpu_device, c["path"][:, lo:hi], w[:, lo:hi], c["starts"][lo:hi], c["ends"][lo:hi],
                                np.array([0, hi - lo]), c["scale"][r:r + 1], can_nmods)
        assert n1[0] == seqlen[r] and s1 == 0
        assert np.array_equal(b1[:n1[0]], buf[int(out_off[r]):int(out_off[r]) + n1[0]]), r


# ----------------------------------------------------------------------------------------------------------------------
# GPU: the dense operator
# ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_extract_mod_weights_one_read_equals_the_reference(gpu_device):
    import torch
    from taiyaki_amd import flipflopfings
    g = _gold()
    for name, can_nmods, T, kind, seed in ms.golden_cases():
        w, path = torch.from_numpy(g[name + "/weights"]).to(gpu_device), torch.from_numpy(g[name + "/path"]).to(gpu_device)
        got = flipflopfings.extract_mod_weights(w, path, can_nmods)
        assert got.is_cuda and got.dtype == torch.float32
        assert ms.same_bits(got.cpu().numpy(), g[name + "/mods"]), name                # row 0 included
    # one column longer than two tiles of the walk: moves at rows 255, 256, 257 and 512, none at 511
    path = ms.flipflop_path(601, 31)
    path[254:258], path[510:513] = [0, 1, 2, 3], [4, 4, 1]
    w = ms.weights((600, 6), 32)
    got = flipflopfings.extract_mod_weights(torch.from_numpy(w).to(gpu_device), torch.from_numpy(path).to(gpu_device),
                                            (1, 1, 0, 0)).cpu().numpy()
    assert np.isnan(got[0]).all() and ms.same_bits(got[1:], ms.moves_to_mods(w, path, (1, 1, 0, 0)))


@pytest.mark.gpu
@pytest.mark.parametrize("ci", range(len(ms.CAN_NMODS)))
def test_extract_mod_weights_batch_equals_the_reference(gpu_device, ci):
    import torch
    from taiyaki_amd import flipflopfings
    g, can_nmods = _gold(), ms.CAN_NMODS[ci]
    names = ["m%d/T%d/%s" % (ci, ms.BATCH_T, kind) for kind in ms.KINDS]
    w = torch.from_numpy(np.stack([g[n + "/weights"] for n in names], axis=1)).to(gpu_device)
    path = torch.from_numpy(np.stack([g[n + "/path"] for n in names], axis=1)).to(gpu_device)
    scores, nbase = flipflopfings.extract_mod_weights(w, path, can_nmods)
    assert nbase.dtype == torch.int32 and nbase.tolist() == [len(g[n + "/mods"]) - 1 for n in names]
    assert nbase.tolist()[1:] == [0, ms.BATCH_T]
    assert ms.same_bits(scores.cpu().numpy(), np.concatenate([g[n + "/mods"][1:] for n in names]))


# ----------------------------------------------------------------------------------------------------------------------
# GPU: whole calls
# ----------------------------------------------------------------------------------------------------------------------
CALL = dict(chunk_size=200, overlap=20, max_concurrent_chunks=4, fastq=True, pack=False)


def _net(which, dev):
    import torch
    from taiyaki_amd import models, synth
    torch.manual_seed(21)
    if which == "lstm":
        net, stride = models.mLstm_cat_mod_flipflop(size=32, stride=5, can_nmods=(1, 1, 0, 0)), 5
    else:
        net, stride = models.mGru_cat_mod_flipflop(size=32, stride=2, can_nmods=(1, 1, 0, 0)), 2
    return synth.excite_network(net).to(dev).eval(), stride        # (as initialised it calls no base)


def _signals(stride):
    rs = np.random.RandomState(41)
    chunk = CALL["chunk_size"] * stride
    # (three chunks, a short read, two chunks, a short read, no samples at all)
    return [(90 + 12 * rs.standard_normal(n)).astype(np.float32) for n in (3 * chunk + 77, chunk // 2 + 3, 2 * chunk - 150, 2, 0)]


def _chain_mods(x, net, stride, dev):
    """One read on the operators the package already had: med / MAD, chunk_read, the network, the posterior
    transition weights, the Viterbi paths of its chunks -- and the restatement on those paths and the network's
    categorical columns."""
    import torch
    from taiyaki_amd import basecall_helpers, clipping, decode
    med, mad = clipping.med_mad(x)
    normed = ((x - med) / mad).astype("f4")
    chunks, starts, ends = basecall_helpers.chunk_read(normed, CALL["chunk_size"] * stride, CALL["overlap"] * stride)
    with torch.no_grad():
        chunks = torch.tensor(chunks, device=dev)
        out = torch.cat([net(c.contiguous()) for c in torch.split(chunks, CALL["max_concurrent_chunks"], 1)], 1)
        trans = (decode.flipflop_make_trans(out[:, :, :40].contiguous()) + 1e-8).log()
        path = decode.flipflop_viterbi_path(trans)
    return ms.stitched_mods(path.cpu().numpy(), out[:, :, 40:].cpu().numpy(), starts, ends, stride, (1, 1, 0, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("which", ["lstm", "gru"])
def test_call_mods_equals_the_chain_of_existing_operators(gpu_device, which, reverse):
    from taiyaki_amd import basecall
    net, stride = _net(which, gpu_device)
    sigs = _signals(stride)
    caller = basecall.Basecaller(net, mod_output=True, reverse=reverse, **CALL)
    assert caller.stride == stride
    results, mods = caller.call_mods(sigs)
    assert results == caller.call(sigs) == basecall.Basecaller(net, reverse=reverse, **CALL).call(sigs)
    assert [r[2] for r in results] == [len(x) for x in sigs] and len(mods) == len(sigs)
    for x, (seq, q, _), m in zip(sigs, results, mods):
        assert m.dtype == np.float32 and m.shape == (len(seq), 2) and len(q) == len(seq)
        if len(x) == 0:                     # (the chain has no network output for a read without samples: no call)
            assert (seq, q) == ("", "") and m.shape == (0, 2)
            continue
        assert ms.same_bits(m, _chain_mods(x[::-1] if reverse else x, net, stride, gpu_device))
        # a row's finite columns are exactly those of its base's modifications (A: column 0, C: column 1)
        letters = np.frombuffer(seq.encode(), dtype=np.uint8)
        assert np.array_equal(~np.isnan(m), np.stack([letters == ord("A"), letters == ord("C")], axis=1))
    print(which, "reverse", reverse, "bases called:", [len(r[0]) for r in results])
    assert min(len(r[0]) for r in results[:3]) > 20                     # (not a comparison of empty calls)


@pytest.mark.gpu
def test_mod_output_false_leaves_call_alone(gpu_device):
    from taiyaki_amd import basecall
    net, stride = _net("lstm", gpu_device)
    sigs = _signals(stride)
    plain = basecall.Basecaller(net, **CALL)
    off = basecall.Basecaller(net, mod_output=False, **CALL)
    assert plain.can_nmods is None and off.can_nmods is None
    want = plain.call(sigs)
    assert off.call(sigs) == want and sum(len(r[0]) for r in want) > 100
    with pytest.raises(RuntimeError, match="mod_output=True"):
        off.call_mods(sigs)
