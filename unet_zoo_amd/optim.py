"""Step tail on flat buffers: ``clip_grad_norm_`` + ``AdamW`` in three kernel launches.

The reference ends every step with ``torch.nn.utils.clip_grad_norm_(model.parameters(), 1.0)`` and
``torch.optim.AdamW.step()`` (unet_zoo/utils/training_loop.py:119-121, optimizer from
scripts/train.py:133).  :class:`FlatClipAdamW` keeps the same arithmetic (decoupled weight decay, bias
corrections, eps outside the square root, the clip coefficient ``min(1, max_norm / (norm + 1e-6))``) but on
ONE flat fp32 buffer per role — parameters, gradients, ``exp_avg``, ``exp_avg_sq`` — so that the gradient
buffer is also what a data-parallel all-reduce moves and what the engine's in-place backward writes.

Parameters are re-pointed at views of the flat parameter buffer (``p.data``) and their ``.grad`` at views
of the flat gradient buffer; only the parameters handed in take part (a parameter the graph never reaches
keeps ``.grad is None`` and is skipped exactly as torch skips it).

:class:`FlatTail` is the same tail with the rate, the step counter and the EMA decay on the device (``uz_steptail.hip``): per-step
schedules, averaged weights and gradient accumulation without host work; :class:`FlatClipAdamW` stays the default.
"""
from __future__ import annotations

import ctypes
from typing import Iterable, List, Optional, Sequence, Tuple

import torch
import torch.nn as nn

from . import _lib as L
from .schedule import LrSchedule


class FlatClipAdamW:
    ALIGN = 64  # elements (256 bytes)

    def __init__(self, params: Iterable[nn.Parameter], lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 1e-2, max_norm: float = 1.0):
        self.params: List[nn.Parameter] = list(params)
        assert self.params, "no parameters"
        dev = self.params[0].device
        L.require_cuda(*self.params)
        self.lr, self.betas, self.eps, self.weight_decay, self.max_norm = lr, betas, eps, weight_decay, max_norm
        # every tensor starts on a 256-byte boundary (kernels read weights / write gradients with 16-byte
        # accesses); the gaps stay zero in all four buffers, so they neither move nor add to the norm
        A = self.ALIGN
        n = sum((p.numel() + A - 1) // A * A for p in self.params)
        self.n = n
        self.flat_p = torch.zeros(n, dtype=torch.float32, device=dev)
        self.flat_g = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros(n, dtype=torch.float32, device=dev)
        self.exp_avg_sq = torch.zeros(n, dtype=torch.float32, device=dev)
        self.step_count = torch.zeros(1, dtype=torch.float32, device=dev)
        off = 0
        self.spans = []
        for p in self.params:
            assert p.dtype == torch.float32
            k = p.numel()
            self.flat_p[off:off + k].copy_(p.detach().reshape(-1))
            p.data = self.flat_p[off:off + k].view_as(p)
            p.grad = self.flat_g[off:off + k].view_as(p)
            self.spans.append((off, off + (k + A - 1) // A * A))
            off += (k + A - 1) // A * A
        wsb = L.load().uz_clip_adamw_workspace_bytes()
        self._ws = torch.empty(wsb // 4, dtype=torch.float32, device=dev)

    def span_of(self, params: Sequence[nn.Parameter]) -> Tuple[int, int]:
        """[begin, end) of a run of consecutive parameters inside the flat buffers"""
        idx = [self.params.index(p) for p in params]
        assert idx == list(range(idx[0], idx[0] + len(idx))), "parameters are not consecutive in the flat order"
        return self.spans[idx[0]][0], self.spans[idx[-1]][1]

    def zero_grad(self) -> None:
        self.flat_g.zero_()

    @torch.no_grad()
    def step(self) -> None:
        L.check(L.load().uz_clip_adamw(self.flat_p.data_ptr(), self.flat_g.data_ptr(), self.exp_avg.data_ptr(),
                                       self.exp_avg_sq.data_ptr(), self.n, self.lr, self.betas[0], self.betas[1],
                                       self.eps, self.weight_decay, self.max_norm, self.step_count.data_ptr(),
                                       self._ws.data_ptr(), L.stream_ptr()), "uz_clip_adamw")

    def last_grad_norm(self) -> torch.Tensor:
        """total gradient norm seen by the last step (before clipping), device scalar"""
        return self._ws[2048 + 3]


def check_tail_args(schedule, ema, accumulate) -> None:
    """the arguments FlatTail adds (GraphedStep checks them when it is built, long before the tail is)"""
    if schedule is not None and not isinstance(schedule, LrSchedule):
        raise TypeError(f"schedule must be a unet_zoo_amd.LrSchedule, got {type(schedule).__name__}")
    if ema is not None and not (isinstance(ema, (int, float)) and not isinstance(ema, bool) and 0.0 <= ema < 1.0):
        raise ValueError(f"ema is the decay of the averaged weights, a number in [0, 1), got {ema!r}")
    if isinstance(accumulate, bool) or not isinstance(accumulate, int) or accumulate < 1:
        raise ValueError(f"accumulate is the number of micro-batches per optimizer step, an int >= 1, got {accumulate!r}")


class FlatTail(FlatClipAdamW):
    """The scheduled step tail (``uz_tail_step``, uz_steptail.hip) on the layout of :class:`FlatClipAdamW`: the same flat
    buffers, ``ALIGN``, ``spans`` and ``span_of``, the same AdamW arithmetic in the same three launches -- with the learning
    rate, the step counter and the EMA decay in a device ``state`` of eight floats (include/unetzoo_hip.h lists them), so that a
    captured ``step()`` follows a per-step :class:`~unet_zoo_amd.schedule.LrSchedule` and a ``set_lr`` without a new capture.

    ema: the decay of an averaged copy of the parameters (``self.ema``, a copy of them to begin with), updated in the apply
    launch: ``e += (1 - d) * (p_new - e)``, d = ema, or ``min(ema, (1 + t) / (10 + t))`` with ema_warmup.  None: no copy.
    accumulate: k > 1 allocates ``self.acc``; ``accumulate_grad(first)`` adds ``flat_g`` into it (one launch) after each of
    the first k - 1 micro-batches, and ``step()`` after the k-th consumes ``(flat_g + acc) / k``: the norm, the clipping and
    AdamW all see the mean gradient.
    With a constant schedule and neither ema nor accumulation the result is bit-identical to :class:`FlatClipAdamW`'s."""

    def __init__(self, params: Iterable[nn.Parameter], lr: float = 1e-3, betas: Tuple[float, float] = (0.9, 0.999),
                 eps: float = 1e-8, weight_decay: float = 1e-2, max_norm: float = 1.0, schedule=None,
                 ema: Optional[float] = None, ema_warmup: bool = True, accumulate: int = 1):
        check_tail_args(schedule, ema, accumulate)
        if schedule is None:
            schedule = LrSchedule.constant()
        super().__init__(params, lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, max_norm=max_norm)
        dev = self.flat_p.device
        self.schedule, self.ema_decay, self.ema_warmup, self.accumulate = schedule, ema, bool(ema_warmup), accumulate
        self.state = torch.zeros(L.TAIL_STATE, dtype=torch.float32, device=dev)
        self.state[L.TAIL_BASE_LR] = lr
        self.step_count = self.state[L.TAIL_T:L.TAIL_T + 1]          # the counter lives in the state
        self.ema = self.flat_p.clone() if ema is not None else None
        self.acc = torch.zeros_like(self.flat_g) if accumulate > 1 else None
        self._ws = torch.empty(L.load().uz_tail_workspace_bytes() // 4, dtype=torch.float32, device=dev)
        d = self.desc = L.TailDesc()
        d.n, d.beta1, d.beta2, d.eps, d.weight_decay, d.max_norm = self.n, betas[0], betas[1], eps, weight_decay, max_norm
        schedule.fill(d)
        d.ema_decay, d.ema_warmup, d.accumulate = (ema if ema is not None else 0.0), int(self.ema_warmup), accumulate

    def set_lr(self, lr: float) -> None:
        """the base rate L of the schedule: a device-side fill of one float, no synchronize"""
        self.lr = lr
        self.state[L.TAIL_BASE_LR].fill_(lr)

    @torch.no_grad()
    def step(self) -> None:
        L.check(L.load().uz_tail_step(ctypes.byref(self.desc), self.flat_p.data_ptr(), self.flat_g.data_ptr(),
                                      self.acc.data_ptr() if self.acc is not None else None, self.exp_avg.data_ptr(),
                                      self.exp_avg_sq.data_ptr(), self.ema.data_ptr() if self.ema is not None else None,
                                      self.state.data_ptr(), self._ws.data_ptr(), L.stream_ptr()), "uz_tail_step")

    @torch.no_grad()
    def accumulate_grad(self, first: bool) -> None:
        """acc = flat_g (first) or acc + flat_g: one launch"""
        L.check(L.load().uz_tail_accumulate(self.acc.data_ptr(), self.flat_g.data_ptr(), self.n, int(bool(first)), L.stream_ptr()),
                "uz_tail_accumulate")

    @torch.no_grad()
    def swap_ema(self) -> None:
        """exchange the CONTENTS of flat_p and ema (one launch): no address moves"""
        L.check(L.load().uz_tail_swap(self.flat_p.data_ptr(), self.ema.data_ptr(), self.n, L.stream_ptr()), "uz_tail_swap")

    def last_grad_norm(self) -> torch.Tensor:
        """norm of the (mean) gradient the last step saw, before clipping, device scalar"""
        return self.state[L.TAIL_NORM]

    def last_lr(self) -> torch.Tensor:
        """the rate the last step used, device scalar"""
        return self.state[L.TAIL_LR]
