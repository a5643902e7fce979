"""Model definitions that feed the flip-flop loss: the reference's
models/mLstm_flipflop.py:6-20, models/mLstm_cat_mod_flipflop.py,
models/mGru_flipflop.py and models/mGru_cat_mod_flipflop.py restated on the PyTorch-ROCm layers of
taiyaki_amd.layers (by scope the RNN stack stays PyTorch)."""
import torch

from taiyaki_amd.layers import (Convolution, GlobalNormFlipFlop, GlobalNormFlipFlopCatMod,
                                GruMod, Lstm, Residual, Reverse, Serial, SquigglePredictor, linear, swish)


def mLstm_flipflop(insize=1, size=256, winlen=19, stride=5, nbase=4):
    return Serial([
        Convolution(insize, 4, 5, stride=1, fun=swish),
        Convolution(4, 16, 5, stride=1, fun=swish),
        Convolution(16, size, winlen, stride=stride, fun=swish),
        Reverse(Lstm(size, size)),
        Lstm(size, size),
        Reverse(Lstm(size, size)),
        Lstm(size, size),
        Reverse(Lstm(size, size)),
        GlobalNormFlipFlop(size, nbase),
    ])


def mLstm_cat_mod_flipflop(insize=1, size=256, winlen=19, stride=5, can_nmods=(1, 1, 0, 0)):
    return Serial([
        Convolution(insize, 4, 5, stride=1, fun=swish),
        Convolution(4, 16, 5, stride=1, fun=swish),
        Convolution(16, size, winlen, stride=stride, fun=swish),
        Reverse(Lstm(size, size)),
        Lstm(size, size),
        Reverse(Lstm(size, size)),
        Lstm(size, size),
        Reverse(Lstm(size, size)),
        GlobalNormFlipFlopCatMod(size, can_nmods),
    ])


def mGru_flipflop(insize=1, size=256, winlen=19, stride=2, nbase=4):
    return Serial([
        Convolution(insize, size, winlen, stride=stride, fun=torch.tanh),
        Reverse(GruMod(size, size)),
        GruMod(size, size),
        Reverse(GruMod(size, size)),
        GruMod(size, size),
        Reverse(GruMod(size, size)),
        GlobalNormFlipFlop(size, nbase),
    ])


def mGru_cat_mod_flipflop(insize=1, size=256, winlen=19, stride=2, can_nmods=(1, 1, 0, 0)):
    return Serial([
        Convolution(insize, size, winlen, stride=stride, fun=torch.tanh),
        Reverse(GruMod(size, size)),
        GruMod(size, size),
        Reverse(GruMod(size, size)),
        GruMod(size, size),
        Reverse(GruMod(size, size)),
        GlobalNormFlipFlopCatMod(size, can_nmods),
    ])


def squiggle_predictor(size=32, depth=4, winlen=9):
    """bin/train_squiggle.py:86-94 (`create_convolution`): per sequence position a level, a log-scale and a move logit
    from the embedded bases, (P, N, 3) -> (P, N, 3).  A `Serial` whose forward also takes `lengths`; on the GPU the
    stack runs as one fused HIP operator (layers.SquiggleNet; the model is a layers.SquigglePredictor)."""
    residual = [Residual(Convolution(size, size, winlen, stride=1, fun=torch.tanh)) for _ in range(depth)]
    return SquigglePredictor([Convolution(3, size, winlen, stride=1, fun=torch.tanh)] + residual
                             + [Convolution(size, 3, winlen, stride=1, fun=linear)])
