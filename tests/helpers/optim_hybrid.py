"""Child process of tests/test_optim.py::test_hybrid_trainer_set_momentum_changes_the_next_replay: a failed hipGraph
capture aborts inside the HIP runtime, so the comparison runs out of process (as tests/helpers/hybrid_vs_eager.py)."""
import copy
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import bench  # noqa: E402  (first: it sets the BLAS environment before torch loads; make_batches)
import torch  # noqa: E402
from taiyaki_amd import _lib, models, optim, parallel, train  # noqa: E402


def _apart(net_a, net_b):
    return max(float((pa - pb).abs().max()) for pa, pb in zip(net_a.parameters(), net_b.parameters()))


def main():
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    _lib.set_strict(False)
    try:
        torch.backends.cuda.preferred_blas_library("cublas")        # = rocBLAS on ROCm (as bench.py)
    except Exception:
        pass
    chunk_len, stride, nbatch, size = 400, 5, 8, 32
    T = chunk_len // stride
    torch.manual_seed(7)
    nets = [models.mLstm_flipflop(size=size, stride=stride).to(dev)]
    nets += [copy.deepcopy(nets[0]), copy.deepcopy(nets[0])]
    batches = bench.make_batches(nbatch, chunk_len, stride, 5, dev, n=3)
    trs = [train.Trainer(n, parallel.FlatGradArena(n), clip_num_mads=0, clip_window=2, hip_optim=True) for n in nets]
    assert all(isinstance(t.opt, optim.FlatAdamW) for t in trs)
    hy_a, hy_b = (train.HybridGraphTrainer(t, batches[0], seq_capacity=nbatch * (T + 1)) for t in trs[:2])
    assert hy_a.alias is None and hy_a.opt is trs[0].opt        # no aliases: the HIP optimiser is captured as it is
    for hy in (hy_a, hy_b):
        hy.load(batches[0])
        hy.capture(warmup=1)        # one eager step + the capture's own tail step, both on batch 0
    eager = trs[2]                  # the same steps by the eager trainer
    la = [float(eager.step(batches[0])), float(eager.step(batches[0]))]
    la.append(float(eager.step(batches[1])))
    lb = float(hy_a.step(batches[1]))
    assert float(hy_b.step(batches[1])) == lb
    torch.cuda.synchronize()
    same = _apart(nets[0], nets[1])
    assert same == 0.0, same        # two hybrid trainers on the same steps
    hy_b.set_momentum(0.5)
    hy_b.set_lr(2e-3)
    eager.opt.set_momentum(0.5)
    eager.opt.set_lr(2e-3)
    hy_a.set_lr(2e-3)
    hy_a.step(batches[2])
    lb2 = float(hy_b.step(batches[2]))
    la.append(float(eager.step(batches[2])))
    torch.cuda.synchronize()
    _lib.raise_if_nonfinite()
    moved = _apart(nets[0], nets[1])                    # beta1 0.9 against 0.5 in the last replay
    like_eager = _apart(nets[1], nets[2])
    steps = [float(t.opt.step_count) for t in trs]
    note = "moved=%.3e like_eager=%.3e loss %.5f / %.5f steps=%s" % (moved, like_eager, lb2, la[-1], steps)
    # the last update is 2e-3 x u, and u with beta1 0.5 is another mean of the same gradients: a hundredth of it at the least;
    # against the eager trainer the bound is that of tests/test_gpu_parity.py's hybrid comparison
    assert moved > 2e-3 * 1e-2 and like_eager < 1e-4 and abs(lb2 - la[-1]) <= 1e-4 * abs(la[-1]), note
    assert steps == [4.0, 4.0, 4.0], note
    cache_note = cache_part(dev, stride, size)
    print("optim-hybrid-ok " + note + " | cache " + cache_note)


def cache_part(dev, stride, size):
    """GraphCacheTrainer on the HIP optimiser over two chunk lengths: the shared optimiser graph (`_opt_step`) replayed
    behind either shape's forward graph, `set_momentum` / `set_lr` before the last step, against the eager trainer."""
    torch.manual_seed(8)
    net_a = models.mLstm_flipflop(size=size, stride=stride).to(dev)
    net_b = copy.deepcopy(net_a)
    lens = [400, 600]
    by_len = {cl: bench.make_batches(int(6 * 600 / cl + 0.5), cl, stride, 5 + cl, dev, n=2) for cl in lens}
    tr_a = train.Trainer(net_a, parallel.FlatGradArena(net_a), clip_num_mads=None, hip_optim=True)
    tr_b = train.Trainer(net_b, parallel.FlatGradArena(net_b), clip_num_mads=None, hip_optim=True)
    maxlen = {cl: max(b["seqlens"].tk_max_seqlen for b in bs) for cl, bs in by_len.items()}
    gc = train.GraphCacheTrainer(tr_b, seq_capacity_per_chunk=lambda cl: cl // stride + 1, max_seqlen_of=lambda cl: maxlen[cl])
    assert gc.alias is None and gc.opt is tr_b.opt
    order = [400, 600, 400, 600, 400]
    worst = 0.0
    for i, cl in enumerate(order):
        if i == len(order) - 1:
            gc.set_momentum(0.5)
            gc.set_lr(2e-3)
            tr_a.opt.set_momentum(0.5)
            tr_a.opt.set_lr(2e-3)
        b = by_len[cl][i % 2]
        la, lb = float(tr_a.step(b)), float(gc.step(b))
        worst = max(worst, abs(la - lb) / max(1e-6, abs(la)))
    torch.cuda.synchronize()
    _lib.raise_if_nonfinite()
    pw = _apart(net_a, net_b)
    steps = [float(tr_a.opt.step_count), float(tr_b.opt.step_count)]
    note = "loss_rel=%.3e param_abs=%.3e graphs=%d steps=%s" % (worst, pw, len(gc.entries), steps)
    # the bound of tests/test_gpu_parity.py's cache-trainer comparison
    assert worst < 1e-4 and pw < 1e-4 and len(gc.entries) == 2 and gc.opt_graph is not None and steps == [5.0, 5.0], note
    assert float(tr_b.opt.hyper[_lib.OPTIM_DEFINES["TK_OPTIM_BETA1"]]) == 0.5
    return note


if __name__ == "__main__":
    main()
