"""The LSTM's parameter gradients on split operands (csrc/lstm_wgrad.hip): every float32 operand is the sum of three
bf16 parts and the product keeps six of the nine part products, on the bf16 matrix cores with float32 accumulation.
What these inputs decide on the device is what the CPU cannot: how the bf16 MFMA rounds inside one instruction, and
that the correction terms are really there.  The criterion is that of tests/test_lstm_wgrad.py: the error against
float64, relative to the largest reference entry, at most twice that of the rocBLAS GEMMs on the same device tensors,
plus 2e-6."""
import functools

import pytest
import torch

from taiyaki_amd import _lib
from tests.test_lstm_wgrad import _case, _errors, _gemms, _kernel

SHAPES = [(13, 20, 128, 128),   # whole tiles (the unguarded loads); K = 260: the last 16-row block is ragged
          (21, 2, 16, 7)]       # the guarded loads


def _reference(dg, x, y):
    """float64 dW_ih, dW_hh, db of float32 host tensors, for both directions."""
    T, N, H = y.shape
    d = dg.double().reshape(T * N, 4 * H)
    ref = {}
    for reverse in (False, True):
        ds, hp = (dg[:-1], y[1:]) if reverse else (dg[1:], y[:-1])
        ref[reverse] = dict(w_ih=d.t() @ x.double().reshape(T * N, -1),
                            w_hh=ds.double().reshape(-1, 4 * H).t() @ hp.double().reshape(-1, H), b=d.sum(0))
    return ref


@functools.lru_cache(maxsize=None)
def _cancelling_case(T, N, H, I):
    """dG[t, n + N/2] = -dG[t, n] and x, y = 1 + 2^-10 randn: the leading parts of x and y are 1 almost everywhere, so
    the products of the leading parts cancel within every time step and dW_ih, dW_hh are made of the correction terms
    (float64: entries of about 2^-10 sqrt(T N), where the summands are of size 1)."""
    g = torch.Generator().manual_seed(77 + T + N + H + I)
    half = torch.randn(T, N // 2, 4 * H, generator=g)
    dg = torch.cat([half, -half], 1).contiguous()
    x = 1 + 2.0 ** -10 * torch.randn(T, N, I, generator=g)
    y = 1 + 2.0 ** -10 * torch.randn(T, N, H, generator=g)
    return dg, x, y, _reference(dg, x, y)


def _compare(name, W, dev, dg, x, y, ref, keys):
    dg, x, y = dg.to(dev), x.to(dev), y.to(dev)
    for reverse in (False, True):
        e_gemm = _errors(_gemms(dg, x, y, reverse), ref[reverse])
        e_hip = _errors(_kernel(W, dg, x, y, reverse), ref[reverse])
        print("%s (T, N, H, I) = %s reverse %d: kernel %s, GEMMs %s"
              % (name, (y.shape[0], y.shape[1], y.shape[2], x.shape[2]), reverse, e_hip, e_gemm))
        for k in keys:
            assert e_hip[k] <= 2 * e_gemm[k] + 2e-6, (name, reverse, k, e_hip[k], e_gemm[k])


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", SHAPES)
def test_cancelling_leading_parts_leave_the_corrections(gpu_device, T, N, H, I):
    """Three products (a1 b1, a1 b2, a2 b1) or five (a2 b2 dropped) miss this by a factor of 5 to 100 (simulated on the
    CPU: 1e-3 to 2e-3 against the float32 GEMM's 1e-4 to 5e-4); six pass (measured: 2.7e-5 to 3.4e-5 against rocBLAS's
    5.5e-5 to 6.9e-5 at the first shape, 4.3e-6 to 5.8e-6 against 1.8e-5 to 2.4e-5 at the second).  db is about 0 here and
    has no scale: tests/test_lstm_wgrad.py covers it."""
    dg, x, y, ref = _cancelling_case(T, N, H, I)
    for t in ref.values():
        assert t["w_ih"].abs().max().item() < 0.05 * dg.abs().max().item() * (T * N) ** 0.5     # (they did cancel)
    _compare("cancelling", _lib.wgrad_lib(), gpu_device, dg, x, y, ref, ("w_ih", "w_hh"))


@pytest.mark.gpu
def test_magnitudes_far_from_one(gpu_device):
    """dG x 1e-6 and x, y x 1e3: the parts are relative to each element, not to the tile."""
    dg, x, y, _ = _case(13, 20, 128, 128)
    dg, x, y = dg * 1e-6, x * 1e3, y * 1e3
    _compare("magnitudes", _lib.wgrad_lib(), gpu_device, dg, x, y, _reference(dg, x, y), ("w_ih", "w_hh", "b"))


@pytest.mark.gpu
@pytest.mark.parametrize("T,N,H,I", SHAPES)
def test_zero_rows_of_dgates_add_exactly_nothing(gpu_device, T, N, H, I):
    """Whole time steps of dG are 0; x there, and the y those steps are multiplied with, are 1e3 in one call and 0 in
    the other: a zero splits into three zeros, so the results are the same bits."""
    W = _lib.wgrad_lib()
    dg, x, y, _ = _case(T, N, H, I)
    zero = [3, 4, 9]
    dg = dg.clone()
    dg[zero] = 0
    for reverse in (False, True):
        outs = []
        for fill in (1e3, 0.0):
            xf, yf = x.clone(), y.clone()
            xf[zero] = fill
            yf[[t + 1 if reverse else t - 1 for t in zero]] = fill
            outs.append(_kernel(W, dg.to(gpu_device), xf.to(gpu_device), yf.to(gpu_device), reverse))
        for k in outs[0]:
            assert bool(torch.isfinite(outs[0][k]).all()) and outs[0][k].abs().max().item() > 0, (reverse, k)
            assert torch.equal(outs[0][k], outs[1][k]), (reverse, k)
