"""Model definitions that feed the flip-flop loss: the reference's
models/mLstm_flipflop.py:6-20, models/mLstm_cat_mod_flipflop.py,
models/mGru_flipflop.py and models/mGru_cat_mod_flipflop.py restated on the PyTorch-ROCm layers of
taiyaki_amd.layers (by scope the RNN stack stays PyTorch)."""
import torch

from taiyaki_amd.layers import (Convolution, GlobalNormFlipFlop, GlobalNormFlipFlopCatMod,
                                GruMod, Lstm, Reverse, Serial, swish)


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
