"""taiyaki_amd.accuracy on the device against tests/align_support.py: exact integer equality, nothing depends on a time."""
import ctypes
import os

import numpy as np
import pytest
import torch

from taiyaki_amd import _lib, accuracy, decode, flipflopfings, models, synth, train
from tests import align_support as support

pytestmark = pytest.mark.gpu

MAX_LEN = _lib.ALIGN_DEFINES["TK_ALIGN_MAX_LEN"]
_FULL = {}


def full(q, r):
    """the support code's full sweep, computed once per pair"""
    key = (support.codes(q).tobytes(), support.codes(r).tobytes())
    if key not in _FULL:
        _FULL[key] = support.align_rows(q, r)
    return _FULL[key]


def words(res):
    """Alignment -> [(distance, matches, exact)] on the host, after checking the derived tensors"""
    d, m, c, e, a = (t.cpu().numpy() for t in res)
    assert d.dtype == m.dtype == c.dtype == e.dtype == np.int32 and a.dtype == np.float32
    assert np.array_equal(c, d + m)
    with np.errstate(invalid="ignore", divide="ignore"):
        assert np.array_equal(a, m.astype(np.float32) / c.astype(np.float32), equal_nan=True)
    return list(zip(d.tolist(), m.tolist(), e.tolist()))


def check_full(qs, rs):
    got = words(accuracy.align_pairs(qs, rs))
    for k, (q, r) in enumerate(zip(qs, rs)):
        assert got[k] == full(q, r) + (1,), (k, len(q), len(r), got[k], full(q, r))
    return got


def instantiation(m, n, t=None):
    out = [ctypes.c_int() for _ in range(3)]
    assert _lib.align_lib().tk_align_band(m, n, -1 if t is None else t, *[ctypes.byref(o) for o in out]) == 0
    return out[2].value


def rand_codes(rng, n, nbase=4):
    return rng.randint(0, nbase, size=n).astype(np.uint8)


def test_empty_and_single_codes(gpu_device):
    qs, rs = zip(*[(q, r) for q in ("", "A", "C") for r in ("", "A", "C")])
    got = check_full(list(qs), list(rs))
    assert got[0] == (0, 0, 1) and got[4] == (0, 1, 1) and got[5] == (1, 0, 1) and got[1] == (1, 0, 1)
    acc = accuracy.align_pairs(list(qs), list(rs)).accuracy.cpu().numpy()
    assert np.isnan(acc[0]) and acc[4] == 1.0 and acc[5] == 0.0
    assert accuracy.align_pairs([], []).distance.shape == (0,)


def test_identical_and_disjoint_sequences(gpu_device):
    rng = np.random.RandomState(3)
    a, b = rand_codes(rng, 300), rand_codes(rng, 211, 2)
    qs, rs = [a, b, b, b + 2, a[:100]], [a, b, b + 2, b[:90], a[:100] + 4]
    got = check_full(qs, rs)
    assert got[0] == (0, 300, 1) and got[2] == (211, 0, 1) and got[3] == (211, 0, 1) and got[4] == (100, 0, 1)


def test_hand_worked_cases_on_the_device(gpu_device):
    qs, rs = ["ACGT", "AAAA", "ACGT", "", "AAC"], ["ACGT", "AAA", "AGCT", "ACG", "ACA"]
    assert check_full(qs, rs) == [(0, 4, 1), (1, 3, 1), (2, 3, 1), (3, 0, 1), (2, 2, 1)]


# every cells-per-lane boundary of the kernel, as widths of a sweep of every diagonal (m + n + 1): the register
# instantiations 1 | 2 | 4 | 8 | 16, the step to the LDS sweep (17) and its first step (19)
BOUNDARIES = [(64, 1), (65, 2), (128, 2), (129, 4), (256, 4), (257, 8), (512, 8), (513, 16), (1024, 16), (1025, 17),
              (1088, 17), (1089, 19)]


def test_lane_strip_boundaries(gpu_device):
    rng = np.random.RandomState(4)
    qs, rs = [], []
    for n in (63, 64, 65, 127, 128, 129):
        r = rand_codes(rng, n)
        qs += [support.mutate(r, 0.1, rng), r[:-1], r]
        rs += [r, r, support.mutate(r, 0.1, rng)]
    for width, cells in BOUNDARIES:
        m, n = (width - 1) // 2, width - 1 - (width - 1) // 2
        assert instantiation(m, n) == cells and instantiation(n, m) == cells, width
        r = rand_codes(rng, n)
        q = support.mutate(r, 0.08, rng)
        q = np.concatenate([q, rand_codes(rng, m)])[:m]
        qs += [q, r]
        rs += [r, q]
    check_full(qs, rs)


def test_band_boundaries_of_long_pairs(gpu_device):
    # the same instantiations reached by a band: t picks the width, the pair is longer than the band is wide
    rng = np.random.RandomState(5)
    r = rand_codes(rng, 1400)
    q = support.mutate(r, 0.03, rng)
    d, mt = full(q, r)
    diff = abs(len(q) - len(r))
    assert d < 150
    # max_distance for a band of `w` diagonals (or w - 1: the band grows two diagonals at a time)
    ts = [diff + 2 * ((w - 1 - diff) // 2) for w in (64, 66, 128, 130, 256, 258, 512, 514, 1024, 1026, 1088, 1090)]
    cells = [instantiation(len(q), len(r), t) for t in ts]
    assert cells == [1, 2, 2, 4, 4, 8, 8, 16, 16, 17, 17, 19], cells
    got = words(accuracy.align_pairs([q] * len(ts), [r] * len(ts), max_distance=ts))
    assert got == [(d, mt, 1)] * len(ts)
    # and below the true distance, at two of them
    low = words(accuracy.align_pairs([q, q], [r, r], max_distance=[max(diff, d - 1), max(diff, d // 2)]))
    assert [g[2] for g in low] == [0, 0] or d - 1 < diff


@pytest.mark.parametrize("rate", [0.0, 0.05, 0.3])
def test_random_pairs(gpu_device, rate):
    rng = np.random.RandomState(int(rate * 100) + 6)
    rs = [rand_codes(rng, n) for n in (400, 457, 512, 555, 600)]
    qs = [support.mutate(r, rate, rng) for r in rs]
    got = check_full(qs, rs)
    if rate == 0.0:
        assert got == [(0, len(r), 1) for r in rs]


def test_tie_breaks_in_runs(gpu_device):
    rng = np.random.RandomState(7)
    homo = lambda n, c=0: np.full(n, c, dtype=np.uint8)                 # noqa: E731
    di = lambda n, s=0: ((np.arange(n) + s) % 2).astype(np.uint8)      # noqa: E731
    qs = [homo(70), homo(70), di(131), di(131), di(200), np.concatenate([homo(40), di(90), homo(33, 1)]), homo(5), di(257)]
    rs = [homo(64), homo(129), di(131, 1), di(140), homo(200), np.concatenate([homo(33), di(99, 1), homo(40, 1)]), di(300),
          np.concatenate([di(100), homo(57), di(100, 1)])]
    qs += [support.mutate(q, 0.1, rng, nbase=2) for q in qs]
    rs += rs
    check_full(qs, rs)


def test_banded_sweeps(gpu_device):
    rng = np.random.RandomState(8)
    qs, rs, ts = [], [], []
    for n, rate in ((60, 0.1), (90, 0.3), (150, 0.05), (150, 0.2), (33, 0.5)):
        r = rand_codes(rng, n)
        q = support.mutate(r, rate, rng)
        if n == 90:
            q = q[:70]                      # a difference in length of its own
        d = full(q, r)[0]
        diff = abs(len(q) - len(r))
        for t in sorted({max(diff - 1, 0), diff, max(d - 2, 0), max(d - 1, 0), d, d + 1, d + 2, d + 9, 4 * d + 100}):
            qs.append(q), rs.append(r), ts.append(t)
    got = words(accuracy.align_pairs(qs, rs, max_distance=ts))
    nexact = 0
    for q, r, t, g in zip(qs, rs, ts, got):
        d, mt = full(q, r)
        assert g[2] == int(d <= t), (len(q), len(r), t, g)             # exact exactly where the true D <= t
        if g[2]:
            assert g[:2] == (d, mt)
        assert g == support.align_banded(q, r, t), (len(q), len(r), t, g)       # ... and the band's own answer elsewhere
        nexact += g[2]
    assert 5 < nexact < len(ts) - 5
    assert any(t < abs(len(q) - len(r)) for q, r, t in zip(qs, rs, ts))
    # one max_distance for all, and the same per pair on the device
    shared = words(accuracy.align_pairs(qs, rs, max_distance=12))
    assert shared == [support.align_banded(q, r, 12) for q, r in zip(qs, rs)]
    dev_t = torch.tensor(ts, dtype=torch.int32, device=gpu_device)
    assert words(accuracy.align_pairs(qs, rs, max_distance=dev_t)) == got
    # align_pairs_exact: the full sweep, whatever the start
    for start in (None, 0, 3):
        res = words(accuracy.align_pairs_exact(qs, rs, start=start))
        assert res == [full(q, r) + (1,) for q, r in zip(qs, rs)], start
    assert accuracy.last_exact["rounds"] > 1


def test_exact_rounds_on_longer_pairs(gpu_device):
    rng = np.random.RandomState(9)
    rs = [rand_codes(rng, n) for n in (900, 1500, 1200)]
    qs = [support.mutate(rs[0], 0.1, rng), support.mutate(rs[1], 0.02, rng), rand_codes(rng, 1100)]
    res = words(accuracy.align_pairs_exact(qs, rs))
    assert res == [full(q, r) + (1,) for q, r in zip(qs, rs)]
    assert accuracy.last_exact["rounds"] >= 2       # (the unrelated pair outgrows every starting band)


def test_length_limit(gpu_device):
    rng = np.random.RandomState(10)
    a = rand_codes(rng, MAX_LEN - 1)
    assert instantiation(len(a), len(a), 8) == 1                        # 9 diagonals: cheap
    assert words(accuracy.align_pairs([a], [a], max_distance=8)) == [(0, MAX_LEN - 1, 1)]
    # beyond it, for lengths only the device sees: reported, not swept
    codes = torch.zeros(MAX_LEN + 1, dtype=torch.uint8, device=gpu_device)
    off = torch.tensor([0, MAX_LEN + 1], dtype=torch.int64, device=gpu_device)
    assert words(accuracy.align_pairs((codes, off), (codes, off), max_distance=8)) == [(MAX_LEN + 1, 0, 0)]


def test_device_tensors_with_offsets(gpu_device):
    rng = np.random.RandomState(11)
    rs = [rand_codes(rng, n) for n in (0, 5, 130, 77)]
    qs = [support.mutate(r, 0.2, rng) for r in rs]
    pack = lambda seqs: (torch.from_numpy(np.concatenate(seqs)).to(gpu_device),                    # noqa: E731
                         torch.from_numpy(np.concatenate([[0], np.cumsum([len(s) for s in seqs])])).to(gpu_device))
    assert words(accuracy.align_pairs(pack(qs), pack(rs))) == [full(q, r) + (1,) for q, r in zip(qs, rs)]
    assert words(accuracy.align_pairs_exact(pack(qs), pack(rs), start=1)) == [full(q, r) + (1,) for q, r in zip(qs, rs)]


def test_mixed_batch_equals_single_launches(gpu_device):
    rng = np.random.RandomState(12)
    lens = np.concatenate([[0, 0, 1, 700, 700], rng.randint(0, 701, size=65)])
    rs = [rand_codes(rng, n) for n in lens]
    qs = [support.mutate(r, rng.choice([0.0, 0.05, 0.3]), rng) for r in rs]
    qs[3], qs[1] = rand_codes(rng, 700), rand_codes(rng, 9)
    assert len(qs) == 70
    got = check_full(qs, rs)
    for k in range(70):
        assert words(accuracy.align_pairs([qs[k]], [rs[k]])) == [got[k]], k


# ---------------------------------------------------------------------------------------------------------------------
# calls against labels
# ---------------------------------------------------------------------------------------------------------------------
def host_chain(path, nbase, seqs, seqlens, lengths=None):
    """download the path, collapse it as path_to_str does, run the support DP"""
    path = path.cpu().numpy()
    out, at = [], 0
    for n, sl in enumerate(seqlens):
        rows = path.shape[0] if lengths is None else int(lengths[n]) + 1
        call = support.collapse(path[:rows, n], nbase)
        alphabet = "".join(chr(65 + b) for b in range(nbase))
        assert "".join(alphabet[c] for c in call) == flipflopfings.path_to_str(path[:rows, n], alphabet)
        out.append(support.align_rows(call, np.asarray(seqs[at:at + sl]) % nbase) + (1,))
        at += sl
    return out


@pytest.mark.parametrize("nbase", [4, 2])
@pytest.mark.parametrize("varlen", [False, True])
def test_call_accuracy_on_iid_scores(gpu_device, nbase, varlen):
    T, N = 50, 9
    S = flipflopfings.nstate_flipflop(nbase)
    sc = torch.from_numpy(synth.scores(T, N, S, 20 + nbase)).to(gpu_device)
    seqlens = np.array([12, 0, 30, 25, 1, 18, 40, 7, 22], dtype=np.int64)
    seqs, _ = synth.sequences(seqlens, 21, nbase=nbase)
    lengths = np.array([50, 37, 0, 1, 50, 49, 13, 25, 8], dtype=np.int64) if varlen else None
    res = accuracy.call_alignment(sc, torch.from_numpy(seqs), torch.from_numpy(seqlens), lengths)
    path = decode.flipflop_viterbi_path(sc, lengths)
    want = host_chain(path, nbase, seqs, seqlens, lengths)
    assert words(res) == want
    acc = accuracy.call_accuracy(sc, torch.from_numpy(seqs), torch.from_numpy(seqlens), lengths)
    assert torch.equal(acc, res.accuracy) and acc.is_cuda
    # labels and counts that already live on the device
    dev = accuracy.call_alignment(sc, torch.from_numpy(seqs).to(gpu_device), torch.from_numpy(seqlens).to(gpu_device),
                                  None if lengths is None else torch.from_numpy(lengths).to(gpu_device))
    assert words(dev) == want


def test_call_accuracy_on_trained_scores(gpu_device):
    sc = np.ascontiguousarray(np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "gru_net_scores0.npz"))["scores/cols_0_8"])
    assert sc.shape == (500, 8, 40)
    seqlens = synth.realistic_seqlens(500, 8, 22, 2000, 9.0).astype(np.int64)
    seqlens[5] = 0
    seqs, _ = synth.sequences(seqlens, 23)
    x = torch.from_numpy(sc).to(gpu_device)
    res = accuracy.call_alignment(x, torch.from_numpy(seqs), torch.from_numpy(seqlens))
    want = host_chain(decode.flipflop_viterbi_path(x), 4, seqs, seqlens)
    assert words(res) == want
    assert max(w[0] + w[1] for w in want) > 200         # (calls of a few hundred bases: the validation shape)


def test_validation_accuracy_ignores_columns_without_labels(gpu_device):
    torch.manual_seed(3)
    net = synth.excite_network(models.mLstm_flipflop(size=32, stride=5)).to(gpu_device).eval()
    N, chunk = 6, 500
    seqlens = np.array([40, 0, 55, 0, 48, 61], dtype=np.int64)
    seqs, _ = synth.sequences(seqlens, 24)
    batch = dict(indata=torch.from_numpy(synth.signal_chunks(chunk, N, 25)).to(gpu_device), seqs=torch.from_numpy(seqs),
                 seqlens=torch.from_numpy(seqlens))
    mean, vec = train.validation_accuracy(net, batch)
    assert mean.is_cuda and vec.shape == (N,) and not mean.requires_grad
    with torch.no_grad():
        out = net(batch["indata"])
    want = host_chain(decode.flipflop_viterbi_path(out), 4, seqs, seqlens)
    want_acc = np.array([m / np.float32(m + d) for d, m, _ in want], dtype=np.float32)
    assert np.array_equal(vec.cpu().numpy(), want_acc)
    live = seqlens > 0
    assert float(mean) == pytest.approx(float(want_acc[live].mean()), rel=1e-6)
    assert not want_acc[~live].any() and float(mean) > float(vec.mean()) > 0      # (a mean over all columns would be lower)
    # with a sample count per column: the varlen forward's rows
    lengths = np.array([500, 500, 305, 120, 500, 40], dtype=np.int64)
    mean_v, vec_v = train.validation_accuracy(net, dict(batch, lengths=lengths))
    from taiyaki_amd import layers
    with torch.no_grad():
        out_v, out_len = layers.forward_varlen(net, batch["indata"], lengths)
    want_v = host_chain(decode.flipflop_viterbi_path(out_v, out_len), 4, seqs, seqlens, out_len)
    want_v = np.array([m / np.float32(m + d) for d, m, _ in want_v], dtype=np.float32)
    assert np.array_equal(vec_v.cpu().numpy(), want_v)
    assert float(mean_v) == pytest.approx(float(want_v[live].mean()), rel=1e-6)
