"""The optimiser step on the device: `FlatAdamW` over a `parallel.FlatGradArena` (include/taiyaki_amd_optim.h,
csrc/optim.hip), the reference's one-cycle schedule as a host object (`OneCycle`, bin/train_flipflop.py:417-429) and the
ab-initio trainer's rolling cap on the gradient's L2 norm (`NormCap`, bin/train_abinitio.py:188-223).

One launch pair replaces the tail of a train step: `arena.finish`'s `mul_`, the gradient maxima and the clamp of
`clipping.DeviceClipper`, the norm cap, AdamW and the `arena.zero()` of the next step.  The hyper-parameters live in a
small device block the kernels read when they run: `set_lr` and `set_momentum` between two replays of a captured step are
what a per-iteration schedule needs (the reference cycles beta1 with `--min_momentum`)."""
import math
import types

import numpy as np
import torch

from taiyaki_amd import _lib

_D = _lib.OPTIM_DEFINES
CU_COUNT = 256          # bounds the grids (8 workgroups per CU); no output depends on it
_GROUP_DEFAULTS = None


def _group_defaults():
    """The keys (and defaults) of a param_group of this torch's AdamW, read off one of its optimisers once."""
    global _GROUP_DEFAULTS
    if _GROUP_DEFAULTS is None:
        _GROUP_DEFAULTS = dict(torch.optim.AdamW([torch.zeros(1, requires_grad=True)], capturable=False).param_groups[0])
    return _GROUP_DEFAULTS


def _check_params(params):
    """TypeError for what the kernels cannot update in place; nothing is changed before it."""
    if len(params) == 0:
        raise TypeError("FlatAdamW: no parameters")
    for i, p in enumerate(params):
        if not p.is_cuda:
            raise TypeError("FlatAdamW: parameter %d is on %s; the update only runs as HIP kernels on an AMD GPU "
                            "(no CPU fallback)" % (i, p.device))
        if p.dtype != torch.float32:
            raise TypeError("FlatAdamW: parameter %d is %s; the kernels update float32" % (i, p.dtype))
        if not p.is_contiguous():
            raise TypeError("FlatAdamW: parameter %d is not contiguous; the kernels write it through a raw pointer" % i)


class FlatAdamW:
    """AdamW (torch.optim.AdamW's arithmetic, decoupled weight decay) over the flat gradient arena, with the scale, the
    clip by value, the L2-norm cap and the zero fill folded in: two launches per step, nothing waits on the host, capturable
    into a hipGraph as a straight chain.

    It owns flat `exp_avg` and `exp_avg_sq` (the arena's layout and offsets), the table of parameter pointers, the tile
    table and the hyper block.  `clipper` (a `clipping.DeviceClipper` on the same arena): the step reads `clipper.thresh`
    and writes `clipper.maxs` in place of `DeviceClipper.launch_kernels()`; `collect()` and `copy_maxima_async()` stay the
    host side of the step.  `max_norm` (None: without a clipper no norm is computed; `float("inf")`: computed, no cap) caps the gradient's L2
    norm as `torch.nn.utils.clip_grad_norm_` does; `grad_norm` is then the norm of the last step, a device scalar.

    The kernels write the parameters through raw pointers, so autograd's version counters do not move.  The contract is the
    one `train._aliased_adamw` relies on: an autograd graph that saved (views of) the parameters may be run backward again
    after a step, and then sees the current weights -- the caller must want that (the hybrid trainers do: their replayed
    forward and eager backward of one step both run between two updates).  Nobody else may hold the parameters' storage to
    a different layout: a parameter that is moved or resized (`module.to`, `p.data = ...`) needs a new FlatAdamW."""

    def __init__(self, arena, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, clipper=None, max_norm=None,
                 amsgrad=False, maximize=False):
        if amsgrad or maximize:
            raise TypeError("FlatAdamW: amsgrad / maximize are not implemented by the kernels")
        if not arena.flat.is_cuda or arena.flat.dtype != torch.float32:
            raise TypeError("FlatAdamW: the gradient arena is %s on %s; the update only runs as HIP kernels on an AMD "
                            "GPU (no CPU fallback)" % (arena.flat.dtype, arena.flat.device))
        params = list(arena.params)
        _check_params(params)
        if clipper is not None and clipper.arena is not arena:
            raise TypeError("FlatAdamW: the clipper belongs to another arena")
        self.arena, self.params, self.clipper = arena, params, clipper
        dev = arena.flat.device
        self.L = _lib.optim_lib()
        off = np.concatenate([[0], np.cumsum([p.numel() for p in params])]).astype(np.int64)
        if int(off[-1]) != arena.flat.numel():
            raise TypeError("FlatAdamW: the arena holds %d elements, its parameters %d" % (arena.flat.numel(), off[-1]))
        self.seg_off = off
        self.nseg, self.total = len(params), int(off[-1])
        self.ntiles = self.L.tk_optim_tile_count(off.ctypes.data, self.nseg)
        if self.ntiles == 0:
            raise ValueError("FlatAdamW: an arena of %d elements is outside the kernels' range" % self.total)
        tiles = np.zeros((self.ntiles, _D["TK_OPTIM_TILE_WORDS"]), dtype=np.uint32)
        _lib.check(self.L.tk_optim_tiles(off.ctypes.data, self.nseg, tiles.ctypes.data, self.ntiles), "tk_optim_tiles")
        self.tiles = torch.from_numpy(tiles.view(np.int32)).to(dev)
        self.ptrs = torch.tensor([p.data_ptr() for p in params], dtype=torch.int64, device=dev)
        self.workspace = torch.zeros(self.L.tk_optim_workspace_bytes(off.ctypes.data, self.nseg), dtype=torch.uint8,
                                     device=dev)
        self.exp_avg = torch.zeros_like(arena.flat)
        self.exp_avg_sq = torch.zeros_like(arena.flat)
        # with a clipper the statistics pass runs anyway: the norm comes with it, and a later set_max_norm needs no new launch form
        self.with_norm = max_norm is not None or clipper is not None
        self._captured_with_norm = None     # the form a captured step() holds
        self.defaults = dict(lr=float(lr), betas=(float(betas[0]), float(betas[1])), eps=float(eps),
                             weight_decay=float(weight_decay))
        host = np.zeros(_D["TK_OPTIM_HYPER_WORDS"], dtype=np.float32)
        host[[_D["TK_OPTIM_LR"], _D["TK_OPTIM_BETA1"], _D["TK_OPTIM_BETA2"], _D["TK_OPTIM_EPS"],
              _D["TK_OPTIM_WEIGHT_DECAY"], _D["TK_OPTIM_GRAD_SCALE"], _D["TK_OPTIM_MAX_NORM"]]] = [
            lr, betas[0], betas[1], eps, weight_decay, 1.0, float("inf") if max_norm is None else max_norm]
        self.hyper = torch.from_numpy(host).to(dev)
        self._grad_scale = 1.0
        self.cu_count = CU_COUNT

    # -- the hyper block: one small fill each ------------------------------------------------------
    def _fill(self, word, value):
        self.hyper[_D[word]:_D[word] + 1].fill_(float(value))

    def set_lr(self, lr):
        self.defaults["lr"] = float(lr)
        self._fill("TK_OPTIM_LR", lr)

    def set_momentum(self, beta1):
        """beta1 of the NEXT step (and of the next replay of a captured one): what OneCycleLR's cycle_momentum sets."""
        self.defaults["betas"] = (float(beta1), self.defaults["betas"][1])
        self._fill("TK_OPTIM_BETA1", beta1)

    def set_max_norm(self, max_norm):
        """The cap of the next step; None or +inf: none.  A FlatAdamW built without `max_norm` and without a clipper computes
        no norm: the first cap switches it on for the steps launched from then on, and raises RuntimeError if a step() was
        captured in the form without a norm (its replays could not follow)."""
        if max_norm is not None and not self.with_norm:
            if self._captured_with_norm is False:
                raise RuntimeError("FlatAdamW.set_max_norm: a step() captured without a norm keeps that form at every replay; "
                                   "build the optimiser with max_norm=float('inf') (or a clipper) before capturing")
            self.with_norm = True
        self._fill("TK_OPTIM_MAX_NORM", float("inf") if max_norm is None else max_norm)

    def set_grad_scale(self, grad_scale):
        """The factor of the next step (a fill only when it changes): set between replays of a captured `step`, it is the
        factor the next replay uses."""
        if float(grad_scale) != self._grad_scale:
            self._fill("TK_OPTIM_GRAD_SCALE", grad_scale)
            self._grad_scale = float(grad_scale)

    @property
    def grad_scale(self):
        return self._grad_scale

    @property
    def grad_norm(self):
        """The L2 norm of the last step's gradients (scaled and clamped, before the cap): a device scalar."""
        return self.hyper[_D["TK_OPTIM_GRAD_NORM"]]

    @property
    def step_count(self):
        """Updates made so far: a device scalar, float32 as torch's capturable step."""
        return self.hyper[_D["TK_OPTIM_STEP"]]

    def step(self, grad_scale=1.0, zero_grads=True):
        """Launches only.  `grad_scale` multiplies the gradients first (1 / (world x sub-batches)); `zero_grads` leaves the
        arena zeroed for the next backward (False: the scaled, clamped, capped gradients stay in it)."""
        self.set_grad_scale(grad_scale)
        if torch.cuda.is_current_stream_capturing():
            self._captured_with_norm = bool(self._captured_with_norm) or self.with_norm
        clip = self.clipper
        with torch.cuda.device(self.arena.flat.device):
            rc = self.L.tk_adamw_step_dev(
                _lib.ptr(self.arena.flat), _lib.ptr(self.exp_avg), _lib.ptr(self.exp_avg_sq), _lib.ptr(self.ptrs),
                _lib.ptr(self.tiles), self.ntiles, self.nseg, self.total, _lib.ptr(self.hyper),
                _lib.ptr(clip.thresh if clip is not None else None), _lib.ptr(clip.maxs if clip is not None else None),
                _lib.ptr(self.workspace), self.workspace.numel(), int(self.with_norm), int(bool(zero_grads)),
                self.cu_count, _lib.stream_ptr())
        _lib.check(rc, "tk_adamw_step_dev")

    # -- checkpoints in torch.optim.AdamW's own layout ------------------------------------------------
    def _group(self):
        g = dict(_group_defaults())
        g.update(lr=self.defaults["lr"], betas=self.defaults["betas"], eps=self.defaults["eps"],
                 weight_decay=self.defaults["weight_decay"], capturable=True, params=list(range(self.nseg)))
        return g

    def state_dict(self):
        """What `torch.optim.AdamW(arena.params, capturable=True).state_dict()` holds after the same steps: per parameter
        `step` (a float32 scalar on the device), `exp_avg`, `exp_avg_sq` (copies, shaped as the parameter); one
        param_group."""
        state = {}
        step = self.hyper[_D["TK_OPTIM_STEP"]]
        for i, (p, lo) in enumerate(zip(self.params, self.seg_off[:-1])):
            lo = int(lo)
            state[i] = dict(step=step.clone(), exp_avg=self.exp_avg[lo:lo + p.numel()].view_as(p).clone(),
                            exp_avg_sq=self.exp_avg_sq[lo:lo + p.numel()].view_as(p).clone())
        return dict(state=state, param_groups=[self._group()])

    def load_state_dict(self, sd):
        groups = sd["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != self.nseg:
            raise ValueError("FlatAdamW.load_state_dict: one param_group of %d parameters expected" % self.nseg)
        g = groups[0]
        if g.get("amsgrad") or g.get("maximize"):
            raise TypeError("FlatAdamW: amsgrad / maximize are not implemented by the kernels")
        state = sd["state"]
        if state and sorted(state) != list(range(self.nseg)):
            raise ValueError("FlatAdamW.load_state_dict: state for parameters %s, expected 0..%d"
                             % (sorted(state), self.nseg - 1))
        steps = {float(s["step"]) for s in state.values()}
        if len(steps) > 1:
            raise ValueError("FlatAdamW.load_state_dict: the parameters' step counts differ (%s)" % sorted(steps))
        for i, (p, lo) in enumerate(zip(self.params, self.seg_off[:-1])):
            if state and tuple(state[i]["exp_avg"].shape) != tuple(p.shape):
                raise ValueError("FlatAdamW.load_state_dict: parameter %d has shape %s, its state %s"
                                 % (i, tuple(p.shape), tuple(state[i]["exp_avg"].shape)))
        self.exp_avg.zero_()
        self.exp_avg_sq.zero_()
        for i, (p, lo) in enumerate(zip(self.params, self.seg_off[:-1])):
            if state:
                lo = int(lo)
                self.exp_avg[lo:lo + p.numel()].copy_(state[i]["exp_avg"].reshape(-1))
                self.exp_avg_sq[lo:lo + p.numel()].copy_(state[i]["exp_avg_sq"].reshape(-1))
        self._fill("TK_OPTIM_STEP", steps.pop() if steps else 0.0)
        betas = tuple(float(b) for b in g["betas"])
        self.defaults.update(betas=betas, eps=float(g["eps"]), weight_decay=float(g["weight_decay"]))
        self.set_lr(float(g["lr"]))
        self.set_momentum(betas[0])
        self._fill("TK_OPTIM_BETA2", betas[1])
        self._fill("TK_OPTIM_EPS", g["eps"])
        self._fill("TK_OPTIM_WEIGHT_DECAY", g["weight_decay"])

    @property
    def param_groups(self):
        """One group, torch's keys.  Read-only (an assignment raises TypeError): the values the kernels use live on the
        device, change them with `set_lr` / `set_momentum` / `set_max_norm`."""
        return (types.MappingProxyType(dict(self._group(), params=tuple(self.params))),)


class OneCycle:
    """`torch.optim.lr_scheduler.OneCycleLR` in its cosine, two-phase form (the one bin/train_flipflop.py:417-429 builds)
    as a host object: `at(i)` is the (lr, beta1) that scheduler has set after i calls of its `step()` -- the values of
    iteration i.  `base_momentum` None: the `cycle_momentum=False` form, beta1 is None."""

    def __init__(self, lr_max, total_steps, pct_start=0.3, div_factor=25.0, final_div_factor=1e4, base_momentum=0.85,
                 max_momentum=0.95):
        if total_steps <= 0 or not 0 <= pct_start <= 1:
            raise ValueError("OneCycle: total_steps %r, pct_start %r" % (total_steps, pct_start))
        self.total_steps = int(total_steps)
        self.initial_lr = lr_max / div_factor
        self.max_lr = lr_max
        self.min_lr = self.initial_lr / final_div_factor
        self.base_momentum, self.max_momentum = base_momentum, max_momentum
        self.ends = (float(pct_start * self.total_steps) - 1, self.total_steps - 1)

    @staticmethod
    def _cos(start, end, pct):
        return end + (start - end) / 2.0 * (math.cos(math.pi * pct) + 1)

    def at(self, i):
        if not 0 <= i <= self.total_steps:
            raise ValueError("OneCycle: iteration %d of %d" % (i, self.total_steps))
        if i <= self.ends[0]:
            pct = (i - 0.0) / (self.ends[0] - 0.0)
            lrs, moms = (self.initial_lr, self.max_lr), (self.max_momentum, self.base_momentum)
        else:
            pct = (i - self.ends[0]) / (self.ends[1] - self.ends[0])
            lrs, moms = (self.max_lr, self.min_lr), (self.base_momentum, self.max_momentum)
        return self._cos(lrs[0], lrs[1], pct), None if self.base_momentum is None else self._cos(moms[0], moms[1], pct)


class NormCap:
    """The ab-initio trainer's cap on the gradient's L2 norm (bin/train_abinitio.py:188-223): every step's uncapped norm
    feeds a `clipping.RollingQuantile`, whose value caps the NEXT step.  The norm travels to the host through a pinned
    asynchronous copy, the data flow `clipping.DeviceClipper` uses for the maxima: `collect()` before a step picks up the
    previous step's norm (its copy finished long ago) and fills the new cap in, `copy_norm_async()` after it starts this
    step's norm on its way."""

    def __init__(self, opt, fraction, window=100):
        from taiyaki_amd import clipping
        self.opt = opt
        self.rolling = clipping.RollingQuantile(fraction, window)
        self.norm_host = torch.zeros(1, dtype=torch.float32).pin_memory()
        self.event = None
        self.last_norm = None
        self.cap = None
        opt.set_max_norm(float("inf"))          # the norm is computed from the first step on; no cap yet

    def collect(self):
        if self.event is None:
            return None
        self.event.synchronize()
        self.event = None
        self.last_norm = float(self.norm_host[0])
        self.cap = float(self.rolling.update(self.last_norm))
        self.opt.set_max_norm(self.cap)
        return self.last_norm

    def copy_norm_async(self):
        with torch.cuda.device(self.opt.arena.flat.device):
            self.norm_host.copy_(self.opt.grad_norm.reshape(1), non_blocking=True)
            self.event = torch.cuda.Event()
            self.event.record()
