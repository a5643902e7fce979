"""Where the projection kernel's weight fragments come from (csrc/rnn_proj.hip): the prep launch writes the three bf16
parts of B into the workspace in fragment order, [column tile][k block][part][32-column block][lane][16 bytes], and
every wave of the main launch reads its own fragments from there.  Two properties, both as bits:

* every fragment lands where it belongs: against a one-hot `a` (row m is 1.0 at k = m, no bias) every product but one
  is an exact zero, so out[m][n] = fl(b1 + fl(b3 + b2)) with b1, b2, b3 the parts of B[n][m] -- a fragment taken from
  the wrong part, 32-column block, k half, k block or column tile is a wrong element;
* the workspace is rewritten by every call and read only after that: three calls on one stream over one workspace with
  weights W1, W2, W1 and no host synchronisation between them each give the bits of a lone call."""
import pytest
import torch

from taiyaki_amd import _lib

CUS = 256
OK = 0


def _call(a, w, bias, grad, out, ws):
    """One call of the entry point on device tensors (a (M, K), w = W_ih (G, I)); nothing waits for it."""
    P = _lib.rnn_proj_lib()
    M, (G, I) = a.shape[0], w.shape
    assert a.shape[1] == (G if grad else I) and out.numel() == M * (I if grad else G)
    if grad:
        rc = P.tk_rnn_input_grad_dev(_lib.ptr(a), _lib.ptr(w), M, I, G, CUS, _lib.ptr(out), _lib.ptr(ws), ws.numel(),
                                     _lib.stream_ptr())
    else:
        rc = P.tk_rnn_input_proj_dev(_lib.ptr(a), _lib.ptr(w), _lib.ptr(bias), M, I, G, CUS, _lib.ptr(out),
                                     _lib.ptr(ws), ws.numel(), _lib.stream_ptr())
    assert rc == OK


def _workspace(I, G, grad, dev, poison):
    """The workspace depends on the widths alone; it is asked for at a number of rows the rule admits."""
    k, nout = (G, I) if grad else (I, G)
    wsb = _lib.rnn_proj_lib().tk_rnn_proj_workspace_bytes(1 << 16, k, nout, CUS)
    assert wsb > 0
    return torch.full((wsb,), poison, dtype=torch.uint8, device=dev)


def _parts_sum(b):
    """fl(b1 + fl(b3 + b2)) of the kernel's split (wgrad_common.h, split2): each part the round-to-nearest-even bf16 of
    what the parts before it left."""
    b1 = b.bfloat16().float()
    r = b - b1
    b2 = r.bfloat16().float()
    b3 = (r - b2).bfloat16().float()
    return b1 + (b3 + b2)


@pytest.mark.gpu
@pytest.mark.parametrize("grad,I,G", [(False, 256, 1024), (False, 96, 288), (False, 16, 48), (True, 256, 1024),
                                      (True, 16, 48)])
def test_every_fragment_lands_where_it_belongs(gpu_device, grad, I, G):
    """Projection (256, 1024): 8 column tiles, 16 blocks; (96, 288): a ragged last column tile, 6 blocks; (16, 48): one
    block, whose successor is the clamped one.  Gradient (256, 1024): 64 blocks, 2 column tiles; (16, 48): 3 blocks, an
    odd count, the clamped one behind the last."""
    K, nout = (G, I) if grad else (I, G)
    g = torch.Generator().manual_seed(100 * I + G + grad)
    w = torch.randn(G, I, generator=g) / K ** 0.5
    B = w.t().contiguous() if grad else w          # (nout, K)
    want = _parts_sum(B).t().contiguous()           # out[m][n] = B[n][m]
    a = torch.eye(K, device=gpu_device)
    out = torch.full((K, nout), float("nan"), device=gpu_device)
    _call(a, w.to(gpu_device), None, grad, out, _workspace(I, G, grad, gpu_device, 0xFF))
    torch.cuda.synchronize()
    got = out.cpu()
    wrong = (got.view(torch.int32) != want.view(torch.int32)).nonzero()
    assert wrong.numel() == 0, "%d wrong elements, the first at (m, n) = %s" % (len(wrong), wrong[0].tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("grad", [False, True])
def test_one_workspace_changing_weights_no_sync_between_calls(gpu_device, grad):
    M, I, G = 129, 256, 1024
    K, nout = (G, I) if grad else (I, G)
    g = torch.Generator().manual_seed(31 + grad)
    a = torch.randn(M, K, generator=g).to(gpu_device)
    w1, w2 = ((torch.randn(G, I, generator=g) / K ** 0.5).to(gpu_device) for _ in range(2))
    bias = None if grad else torch.randn(G, generator=g).to(gpu_device)
    lone = []
    for w, poison in ((w1, 0xFF), (w2, 0x3F)):
        out = torch.full((M, nout), float("nan"), device=gpu_device)
        _call(a, w, bias, grad, out, _workspace(I, G, grad, gpu_device, poison))
        torch.cuda.synchronize()
        lone.append(out)
    assert not torch.equal(lone[0], lone[1])
    ws = _workspace(I, G, grad, gpu_device, 0xFF)
    outs = [torch.full((M, nout), float("nan"), device=gpu_device) for _ in range(3)]
    torch.cuda.synchronize()
    for w, out in zip((w1, w2, w1), outs):
        _call(a, w, bias, grad, out, ws)
    torch.cuda.synchronize()
    for i, (out, ref) in enumerate(zip(outs, (lone[0], lone[1], lone[0]))):
        assert torch.equal(out.view(torch.int32), ref.view(torch.int32)), "call %d" % i
