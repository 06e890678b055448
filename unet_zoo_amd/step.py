"""The reference's training step as hipGraph replays: ``GraphedStep``.

The reference's hot loop (unet_zoo/utils/training_loop.py:108-124) is, per batch,

    optimizer.zero_grad(); outputs = model(img); loss, dice = criterion(...); loss.backward()
    clip_grad_norm_(model.parameters(), 1.0); optimizer.step()

Launched eagerly from Python this engine is CPU-bound (17.7 ms of launches for 10 ms of GPU work on the UNet of
BASELINE configs[1]).  ``GraphedStep`` is the same step captured once and replayed:

    step = unet_zoo_amd.GraphedStep(model, lr=1e-4, weight_decay=1e-5)     # instead of optim.AdamW(...)
    loss = step(img, mask)                                                 # instead of lines 112-121
    outputs, dice = step.outputs, step.dice                                # device tensors, no host sync

* hipGraph 1..K: forward + loss + backward, the backward cut into K phases at tape positions; every kernel writes
  its parameter gradient in place into ONE flat fp32 buffer laid out phase by phase;
* with more than one rank (one process per GPU, ``torch.distributed`` over RCCL): after phase k's graph its span of
  the flat buffer is all-reduced (AVG, asynchronous) while phase k+1's graph runs — collectives stay outside graph
  capture and still overlap the backward (replaces ``nn.DataParallel``, multi_gpu.py:20-31);
* last hipGraph: ``clip_grad_norm_(max_norm)`` + AdamW on the flat parameter / gradient / moment buffers (three
  launches, ``optim.FlatClipAdamW``).

``step.loss``, ``step.dice`` and ``step.outputs`` are STATIC tensors of the captured graphs: the next call overwrites
them in place, so read (``.item()``) or ``.clone()`` what must outlive the step.

Loss: the default ``criterion="bce_dice"`` is the fused kernel of ``loss.py`` (BCEWithLogits + its gradient + the
Dice metric, one pass) inside the first graph.  Any ``criterion.FusedCriterion`` (``RegionLoss``: BCE + soft Dice / Tversky /
focal Tversky, weighted over the output maps; ``MulticlassLoss``: softmax cross-entropy + Dice over class-index labels; the
criteria composed on them) sits in the same place: its launches inside the first graph, ``step.dice`` keeps its meaning;
with several ranks each rank evaluates it on its own shard, so ``reduce="batch"`` is per shard.  The static target
buffer has the criterion's ``target_dtype``: int32 for class-index labels, float32 for every other criterion.  Any other
callable ``criterion(outputs, target) -> loss`` works too; it is evaluated EAGERLY between the forward graph and the
backward graphs, because library reductions must not be captured on this stack: a memset node of a replayed hipGraph writes its value only in the first replay, and torch's multi-block
reductions reset their semaphores with exactly such a node (tools/graph_canary.py).

Augmentation: ``GraphedStep(model, augment=unet_zoo_amd.GpuAugment(...))`` copies the caller's batch into static RAW buffers and
captures the augmentation's two launches (``uz_augment.hip``) at the head of the first graph -- the forward graph on the eager-
criterion route, phase 0 on the fused-loss route; the model and the criterion read the augmentation's static outputs
(``step.augmented``).  Its draws are torch's generator's, so every replay draws afresh and a seed reproduces a run; with several
ranks each rank draws from its OWN generator (seed the ranks differently unless they are meant to augment alike).  Without
``augment`` nothing changes: the same graphs, the same buffers, the same numbers.

Patches from a device pool: ``GraphedStep(model, crit, source=unet_zoo_amd.PatchSampler(...))`` takes NO batch -- ``loss = step()``.
The sampler's two launches (``uz_patch.hip``: draw the windows, cut them out) are captured at the head of the first graph, in
front of the augmentation's when there is one, which then reads the sampler's static outputs as its raw batch; every replay
draws its own patches (``step.sampled``, ``step.coords``) and the host does nothing per step.  The dry run that plans the graphs
needs real patches, so ONE set of draws is consumed before the capture (with ``force_draws(u)`` that is not sticky, the forced
ones).  With several ranks each rank holds its own pool and draws from its own generator.  Without ``source`` nothing changes.

The scheduled tail: ``GraphedStep(model, schedule=LrSchedule.cosine(10_000, warmup_steps=500), ema=0.999, accumulate=2)``.  Any of
``schedule`` / ``ema`` / ``accumulate`` replaces the last hipGraph's three launches by ``optim.FlatTail``'s (``uz_steptail.hip``):
the same clip + AdamW arithmetic, with the step counter, the BASE rate and the rate in use in a device state.
* ``schedule``: the prepare launch evaluates the schedule from the device's counter, every replay at its own rate; ``set_lr(lr)``
  fills the base rate on the stream -- no synchronize, no new capture; ``step.lr_now`` is the rate the last step used.
* ``ema``: an averaged copy of the weights, updated in the apply launch (``ema_warmup``: decay ``min(ema, (1 + t) / (10 + t))``);
  ``with step.ema_weights():`` exchanges its contents with the parameters' for evaluation and saving.  BatchNorm running
  statistics are module buffers: shared, not averaged.
* ``accumulate=k``: one optimizer step takes k calls of ``step(x, t)``; calls 1 .. k-1 replay the forward / backward graphs and add
  the gradient to an accumulator (one eager launch), call k replays a tail that consumes ``(flat_g + acc) / k``.  Every call
  returns its own micro-batch loss, ``grad_norm`` is the norm of the mean gradient, ``steps_done`` counts optimizer steps, BatchNorm
  running statistics advance per micro-batch as in torch.  With several ranks the per-phase all-reduce runs in EVERY micro-step:
  the mean is linear, so the result is right, but k - 1 of the k exchanges could be saved -- not optimised.
* ``step.state_dict()`` / ``load_state_dict()``: the moments, the counter, the rate, the position inside an accumulation and the
  EMA / accumulator buffers by parameter name -- with ``checkpoint.save_model_state`` a run resumes bit for bit (both tails).
With all of them at their defaults nothing changes: the same class, the same graphs, ``set_lr`` captures the tail again.
"""
from __future__ import annotations

import contextlib
from collections import OrderedDict
from typing import Callable, Dict, List, Optional, Sequence, Tuple, Union

import torch
import torch.distributed as dist
import torch.nn as nn

from .graph import PhasedStep
from .augment import GpuAugment
from .patches import PatchSampler
from .capture import CAPTURE_MODE, _check_capture, _new_graph, _unwrap, resolve_criterion, static_copy, unchanged
from .criterion import FusedCriterion
from .optim import FlatClipAdamW, FlatTail, check_tail_args
from .schedule import LrSchedule


class _ShapeGraphs:
    """everything captured for one (input shape, target shape): x / t take the caller's batch, mx / mt are what the model and
    the criterion read -- the same tensors, or the static outputs of the augmentation `aug` captured in front of the model;
    src: the patch sampler captured in front of both, whose static outputs are then x / t"""
    __slots__ = ("x", "t", "mx", "mt", "aug", "src", "fwd", "phases", "gouts", "loss", "dice", "outputs", "pool", "ps", "tables")


class GraphedStep:
    def __init__(self, model: nn.Module, criterion: Union[str, FusedCriterion, Callable] = "bce_dice", *, lr: float = 1e-4,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 1e-5,
                 max_norm: float = 1.0, phases: int = 5, process_group=None, data_parallel: Optional[bool] = None,
                 cu_reserve: Optional[int] = None, comm: str = "overlap", comm_dtype: Optional[torch.dtype] = None,
                 augment: Optional[GpuAugment] = None, source: Optional[PatchSampler] = None,
                 schedule: Optional[LrSchedule] = None, ema: Optional[float] = None, ema_warmup: bool = True,
                 accumulate: int = 1):
        """schedule / ema / ema_warmup / accumulate: the scheduled step tail (module docstring); with all four at their defaults
        the tail is FlatClipAdamW as before.
        augment: a GpuAugment applied to every batch inside the first graph (module docstring); every rank draws from its own
        generator.
        source: a PatchSampler whose patches ARE the batch: the step is then called without arguments (module docstring).
        comm: when the gradient exchange of a data-parallel step runs -- "overlap": the span of every finished backward
        phase is all-reduced while the next phase's graph runs; "tail": ONE all-reduce of the whole flat buffer after the
        last phase.  The same graphs serve both; autotune_comm() times them on the job's own hardware and keeps the faster
        one (the persistent one-workgroup-per-CU grids and a collective's kernels compete for CUs: which schedule wins
        depends on the rank count and the fabric).
        comm_dtype: None / torch.float32 -- gradients are all-reduced in fp32 (the reference's DataParallel sums fp32 replicas'
        gradients, multi_gpu.py:28-31); torch.bfloat16 -- an OPTION that halves the bytes on the links: every rank rounds its
        span to bf16, a reduce-scatter by all-to-all, the shards are summed in fp32 ON ARRIVAL (fixed rank order) and averaged,
        rounded once to bf16 and all-gathered: every rank ends with the same bf16-representable mean; 2 (N-1)/N of the bf16
        span crosses each rank's links instead of 2 (N-1)/N of the fp32 one, and the direct all-to-all / all-gather pair uses
        all of a GPU's xGMI links at once.  Not the default: it changes the gradients by two bf16
        roundings.
        cu_reserve: CUs the library's persistent grids leave free (uz_set_cu_reserve; process-wide, applied here,
        before anything is planned or captured) so that the all-reduce of a finished gradient span can start while the
        next backward phase runs -- convolution / GEMM / weight-gradient kernels otherwise hold every CU with one
        160 KB workgroup until a kernel boundary.  None leaves the library's setting alone (default 0)."""
        self.model = _unwrap(model)
        if cu_reserve is not None:
            from . import _lib
            _lib.set_cu_reserve(cu_reserve)
        fused, self._target_dtype = resolve_criterion(criterion)
        self._fused, self._fused_loss = fused, fused is not None
        # (the lambda must not close over self: in a reference cycle this object and its hipGraphs would wait for the garbage
        # collector, which may then destroy them in the middle of somebody's capture)
        self._loss_fn = (lambda out, t: fused[0](out, t)[0]) if fused is not None else criterion
        if augment is not None and not isinstance(augment, GpuAugment):
            raise TypeError(f"augment must be a unet_zoo_amd.GpuAugment, got {type(augment).__name__}")
        self.augment = augment
        if source is not None and not isinstance(source, PatchSampler):
            raise TypeError(f"source must be a unet_zoo_amd.PatchSampler, got {type(source).__name__}")
        if source is not None and source.out_mask is None:
            raise ValueError("source: the PatchSampler has no masks, a training step needs targets")
        if source is not None and source.out_mask.dtype != self._target_dtype:
            raise ValueError(f"source: the PatchSampler yields {source.out_mask.dtype} masks, the criterion takes {self._target_dtype} "
                             "targets (class indices go with MulticlassLoss, fp32 masks with every other criterion)")
        self.source = source
        self.lr, self.betas, self.eps, self.weight_decay, self.max_norm = lr, betas, eps, weight_decay, max_norm
        check_tail_args(schedule, ema, accumulate)
        self.schedule, self.ema_decay, self.ema_warmup, self.accumulate = schedule, ema, bool(ema_warmup), accumulate
        # any of the three given: the tail is FlatTail (uz_steptail.hip); none: FlatClipAdamW, exactly as before
        self._tail = schedule is not None or ema is not None or accumulate != 1
        self._micro = 0                      # micro-batches already accumulated towards the next optimizer step
        self._in_ema = False                 # inside `with step.ema_weights():`
        self._pending_state: Optional[dict] = None
        self.pg = process_group
        self.world = dist.get_world_size(process_group) if dist.is_initialized() else 1
        # data_parallel=True with one rank keeps the multi-rank launch strategy (phases + collectives): a rehearsal
        self.distributed = (self.world > 1) if data_parallel is None else bool(data_parallel)
        if self.distributed and not dist.is_initialized():
            raise RuntimeError("data_parallel=True needs an initialised torch.distributed process group")
        self._nccl = self.distributed and dist.get_backend(process_group) == "nccl"
        self.n_phases = max(1, int(phases)) if self.distributed else 1
        if comm not in ("overlap", "tail"):
            raise ValueError(f"comm must be 'overlap' or 'tail', got {comm!r}")
        self.comm = comm
        if comm_dtype not in (None, torch.float32, torch.bfloat16):
            raise ValueError(f"comm_dtype must be None, torch.float32 or torch.bfloat16, got {comm_dtype!r}")
        self.comm_dtype = torch.bfloat16 if comm_dtype == torch.bfloat16 else torch.float32
        self._comm_stream: Optional[torch.cuda.Stream] = None
        self._comm_bufs: Dict[tuple, tuple] = {}
        self.opt: Optional[FlatClipAdamW] = None
        self._g_opt: Optional[torch.cuda.CUDAGraph] = None
        self._cuts: Optional[List[int]] = None
        self._spans: List[Tuple[int, int]] = []
        self._graphs: Dict[tuple, _ShapeGraphs] = {}
        self._cur: Optional[_ShapeGraphs] = None
        self.loss: Optional[torch.Tensor] = None
        self.dice: Optional[torch.Tensor] = None
        self.outputs = None
        self.steps_done = 0

    # ------------------------------------------------------------------ set-up (first call)
    def _dry_run(self, x: torch.Tensor, t: torch.Tensor):
        """One eager forward + backward that changes nothing: finds the parameters the graph reaches, the tape
        position that completes each of them, and warms the weight-layout cache."""
        m = self.model
        for p in m.parameters():
            p.grad = None
        ps = PhasedStep(m, self._loss_fn)
        with unchanged(m, x.device):
            ps.forward(x, t)
            ps.backward(ps.n_entries, 0, True)
            K = self.n_phases
            # cut where the cumulative gradient bytes cross k/(K-1) * 85 %: the last phase (the high-resolution
            # layers: few parameters, long compute) hides the exchange of everything before it
            fr = [0.85 * (i + 1) / (K - 1) for i in range(K - 1)] if K > 1 else []
            cuts, groups = ps.plan(fr)
            ps.finish()
        return cuts, groups

    def _setup(self, x: torch.Tensor, t: torch.Tensor) -> None:
        m = self.model
        if not m.training:
            raise RuntimeError("GraphedStep is the TRAINING step: call model.train() first "
                               "(evaluate with model.eval() and torch.no_grad() as the reference does)")
        cuts, groups = self._dry_run(x, t)
        ordered = [p for grp in groups for p in grp]
        if not ordered:
            raise RuntimeError("no parameter received a gradient")
        if self._tail:
            self.opt = FlatTail(ordered, lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                                max_norm=self.max_norm, schedule=self.schedule, ema=self.ema_decay, ema_warmup=self.ema_warmup,
                                accumulate=self.accumulate)
        else:
            self.opt = FlatClipAdamW(ordered, lr=self.lr, betas=self.betas, eps=self.eps,
                                     weight_decay=self.weight_decay, max_norm=self.max_norm)
        # the parameters moved into the flat buffer: new pointer tables, built outside any capture
        m._pack_cache.repoint()
        m._pack_cache.refresh(m.run_dtype)
        A, off = FlatClipAdamW.ALIGN, 0
        self._spans = []
        for grp in groups:
            k = sum((p.numel() + A - 1) // A * A for p in grp)
            self._spans.append((off, off + k))
            off += k
        assert off == self.opt.n
        self._cuts = cuts
        if self.world > 1:
            # every rank starts from rank 0's parameters and buffers (one collective for all parameters); BatchNorm
            # running statistics then follow each rank's own shard, as the reference's DataParallel replicas do
            self._broadcast(self.opt.flat_p)
            for b in m.buffers():
                self._broadcast(b)
        if self._pending_state is not None:      # a load_state_dict() from before the flat buffers existed
            state, self._pending_state = self._pending_state, None
            self._apply_state(state)
        self._capture_opt()

    def _capture_opt(self) -> None:
        self._g_opt = _new_graph()
        with torch.cuda.graph(self._g_opt, capture_error_mode=CAPTURE_MODE):
            self.opt.step()
        _check_capture(self._g_opt, "optimizer graph")

    def set_lr(self, lr: float) -> None:
        """Learning-rate change (the reference's DiceScheduler, utils/lr_scheduler.py:70-81).  Default tail: the rate is a
        kernel argument, so the three-launch optimizer graph is captured again.  Scheduled tail: the BASE rate of the
        schedule is one device float (state[1]); it is filled on the stream -- no synchronize, no new capture."""
        self.lr = lr
        if self.opt is None:
            return
        if self._tail:
            self.opt.set_lr(lr)
        else:
            self.opt.lr = lr
            torch.cuda.synchronize()
            self._capture_opt()

    def _capture(self, x: torch.Tensor, t: torch.Tensor, aug=None, src=None) -> _ShapeGraphs:
        """x, t: the static tensors the model and the criterion read; aug: the bound augmentation that writes them (its two
        launches open the first graph) or None; src: the bound patch sampler whose two launches come in front of those, or None"""
        g = _ShapeGraphs()
        g.x, g.t, g.mx, g.mt, g.aug, g.src = x, t, x, t, aug, src
        ps = PhasedStep(self.model, self._loss_fn)
        cuts = self._cuts
        g.phases, g.fwd, g.gouts, g.dice, pool = [], None, None, None, None
        torch.cuda.synchronize()
        if self._fused_loss:
            dice_box = []
            with_autograd, direct = self._fused

            def fused(out, tt):
                l, d = with_autograd(out, tt)
                dice_box.append(d)
                return l

            def fused_direct(out, tt):   # the same numbers and d(loss)/d(outputs) without autograd's three extra launches
                l, d, gouts = direct(out, tt)
                dice_box.append(d)
                return l, gouts
            fused.direct = fused_direct
            ps.loss_fn = fused
        else:
            # forward graph; the criterion runs eagerly on its static outputs; the backward graphs read static
            # d(loss)/d(output) buffers
            g.fwd = _new_graph()
            with torch.cuda.graph(g.fwd, capture_error_mode=CAPTURE_MODE):
                if src is not None:
                    src.run()
                if aug is not None:
                    aug.run()
                ps.emit(g.mx)
            _check_capture(g.fwd, "forward graph")
            pool = g.fwd.pool()
            g.outputs = ps.outputs
            g.gouts = [torch.zeros_like(o) for o in ps._outs]
            ps.set_output_grads(g.gouts)
        for k in range(len(cuts) - 1):
            gk = _new_graph()
            with torch.cuda.graph(gk, pool=pool, capture_error_mode=CAPTURE_MODE):
                if k == 0 and self._fused_loss:
                    if src is not None:
                        src.run()
                    if aug is not None:
                        aug.run()
                    g.loss = ps.forward(g.mx, g.mt)
                    g.outputs = ps.outputs
                    g.dice = dice_box[-1].detach()
                ps.backward(cuts[k], cuts[k + 1], k == 0)
            _check_capture(gk, f"backward phase {k}")
            pool = gk.pool()
            g.phases.append(gk)
        g.ps = ps            # keeps the loss function / output leaves for the eager criterion
        if self._fused_loss:
            ps.finish()
        else:
            ps.eng.tape.clear()
            ps.eng = None
        g.pool = pool
        # the graphs hold the pack cache's pointer tables by address, and nothing captures them again: keep THESE tables alive.
        # The cache drops its own references when it builds new ones (a new weight copy; a graphed inference runner of this
        # model that saw the storage move, capture.GraphedRunner._lookup), and a replay must not read freed memory.
        c = self.model._pack_cache
        g.tables = (c._table, c._table3)
        return g

    # ------------------------------------------------------------------ collectives
    def _broadcast(self, t: torch.Tensor) -> None:
        if self._nccl:
            dist.broadcast(t, src=0, group=self.pg)
        else:
            h = t.detach().cpu()
            dist.broadcast(h, src=0, group=self.pg)
            t.copy_(h)

    class _EventWait:
        """what the bf16 exchange hands back in place of a collective's work handle"""

        def __init__(self, ev):
            self.ev = ev

        def wait(self):
            torch.cuda.current_stream().wait_event(self.ev)

    def _exchange_bf16(self, buf: torch.Tensor):
        """buf (a span of the flat fp32 gradient buffer) <- bf16(mean over ranks of bf16(buf)): all-to-all of bf16 shards,
        fp32 sum on arrival in rank order, one rounding, all-gather -- on a side stream, so that the next backward phase
        keeps running; returns an object whose wait() orders the caller's stream behind it"""
        n, W = buf.numel(), self.world
        shard = (n + W - 1) // W
        key = (buf.data_ptr(), n)
        if key not in self._comm_bufs:
            dev = buf.device
            self._comm_bufs[key] = (torch.zeros(W * shard, dtype=torch.bfloat16, device=dev),
                                    torch.empty(W * shard, dtype=torch.bfloat16, device=dev),
                                    torch.empty(shard, dtype=torch.bfloat16, device=dev))
        send, recv, mine = self._comm_bufs[key]
        if self._comm_stream is None:
            self._comm_stream = torch.cuda.Stream(device=buf.device)
        ready = torch.cuda.Event()
        ready.record()
        cs = self._comm_stream
        with torch.cuda.stream(cs):
            cs.wait_event(ready)
            send[:n].copy_(buf)                                   # fp32 -> bf16 (round to nearest even); the tail stays zero
            dist.all_to_all_single(recv, send, group=self.pg)     # shard r of every rank's span arrives at rank r
            mine.copy_(recv.view(W, shard).float().sum(0).mul_(1.0 / W))   # fp32 accumulate on arrival, fixed order, one rounding
            dist.all_gather_into_tensor(send, mine, group=self.pg)
            buf.copy_(send[:n])
            done = torch.cuda.Event()
            done.record(cs)
        return GraphedStep._EventWait(done)

    def _all_reduce_avg(self, buf: torch.Tensor):
        if self.comm_dtype == torch.bfloat16:
            if self._nccl:
                return self._exchange_bf16(buf)
            # other backends (gloo rehearsals): the same arithmetic staged through the host -- every rank's span rounded to
            # bf16, summed in fp32, averaged, rounded once
            h = buf.detach().to(torch.bfloat16).float().cpu()
            dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.pg)
            buf.copy_(h.mul_(1.0 / self.world).to(torch.bfloat16).float().to(buf.device))
            return None
        if self._nccl:
            return dist.all_reduce(buf, op=dist.ReduceOp.AVG, group=self.pg, async_op=True)
        # other backends (gloo: CPU rehearsals and the single-GPU two-rank test): staged through the host
        h = buf.detach().cpu()
        dist.all_reduce(h, op=dist.ReduceOp.SUM, group=self.pg)
        buf.copy_(h.mul_(1.0 / self.world).to(buf.device))
        return None

    # ------------------------------------------------------------------ the step
    def forward_backward(self, x: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None) -> torch.Tensor:
        """zero_grad + forward + loss + backward (+ gradient all-reduce): afterwards every ``p.grad`` (views of the flat
        buffer) holds this step's (rank-averaged) gradient.  Returns the loss as a device scalar.  With `source` the batch
        is the sampler's and no argument is taken."""
        self._refuse_in_ema()
        if self.source is not None:
            if x is not None or target is not None:
                raise TypeError("this GraphedStep draws its batch from `source` (a PatchSampler): call it without arguments")
            key = ("source",)
        elif x is None or target is None:
            raise TypeError("GraphedStep takes a batch (x, target); only a step built with source= is called without one")
        else:
            key = (tuple(x.shape), tuple(target.shape))
        g = self._graphs.get(key)
        if g is None:
            dev = next(self.model.parameters()).device
            src = None
            if self.source is not None:
                # the sampler's static outputs are the raw buffers; the dry run needs real patches: one set of draws is consumed
                src = self.source.bind()
                if src.out_image.device != dev:
                    raise ValueError(f"source: the PatchSampler's pool is on {src.out_image.device}, the model on {dev}")
                sx, st = src.run()
            else:
                # static input buffers of this shape (training_loop.py:109-110)
                sx, st = static_copy(x, dev), static_copy(target, dev, self._target_dtype)
            aug, mx, mt = None, sx, st
            if self.augment is not None:
                # the augmentation reads the raw copies and writes static outputs of its own; for the dry run they hold the
                # raw batch (nothing is drawn before the capture, the generator is where the caller left it)
                sx, st = sx.contiguous(), st.contiguous()      # bind() reads these very tensors in place
                aug = self.augment.bind(sx, st)
                mx, mt = aug.out_image, aug.out_mask
                mx.copy_(sx)
                mt.copy_(st)
            if self.opt is None:
                self._setup(mx, mt)
            g = self._graphs[key] = self._capture(mx, mt, aug, src)
            g.x, g.t = sx, st
        self._cur = g
        if g.src is None:
            if x.data_ptr() != g.x.data_ptr():
                g.x.copy_(x)
            if target.data_ptr() != g.t.data_ptr():
                g.t.copy_(target)
        if g.fwd is not None:
            g.fwd.replay()
            loss = g.ps.loss(g.mt)                   # eager criterion; leaves d(loss)/d(output)
            for dst, src in zip(g.gouts, g.ps._gouts):
                if src is None:
                    dst.zero_()
                else:
                    dst.copy_(src)
            self.loss = loss
        else:
            self.loss = g.loss
        self.dice, self.outputs = g.dice, g.outputs
        if self.distributed and self.comm == "tail":
            for gk in g.phases:
                gk.replay()
            w = self._all_reduce_avg(self.opt.flat_g[:self._spans[-1][1]])
            if w is not None:
                w.wait()
        elif self.distributed:
            works = []
            for gk, (a0, a1) in zip(g.phases, self._spans):
                gk.replay()
                works.append(self._all_reduce_avg(self.opt.flat_g[a0:a1]))
            for w in works:
                if w is not None:
                    w.wait()
        else:
            for gk in g.phases:
                gk.replay()
        return self.loss

    def autotune_comm(self, x: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None, steps: int = 6) -> Dict[str, float]:
        """Time `steps` whole training steps under each collective schedule ("overlap", "tail") on this job's ranks and
        keep the faster one; every rank takes the same decision (the slowest rank's time counts).  These are real
        optimizer steps on (x, target).  Returns {"overlap": ms, "tail": ms}."""
        if not self.distributed:
            return {}
        dev = next(self.model.parameters()).device
        out: Dict[str, float] = {}
        for mode in ("overlap", "tail"):
            self.comm = mode
            for _ in range(2):
                self(x, target)
            torch.cuda.synchronize(dev)
            if self.world > 1:
                dist.barrier(group=self.pg)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(steps):
                self(x, target)
            e1.record()
            torch.cuda.synchronize(dev)
            ms = torch.tensor([e0.elapsed_time(e1) / steps], dtype=torch.float64, device=dev if self._nccl else "cpu")
            if self.world > 1:
                dist.all_reduce(ms, op=dist.ReduceOp.MAX, group=self.pg)
            out[mode] = float(ms.item())
        self.comm = "tail" if out["tail"] < 0.99 * out["overlap"] else "overlap"      # overlap unless the tail schedule wins by > 1 %
        return out

    def optimizer_step(self) -> None:
        """clip_grad_norm_(max_norm) + AdamW on the flat buffers (training_loop.py:120-121)"""
        self._refuse_in_ema()
        self._g_opt.replay()
        self.steps_done += 1
        self._micro = 0

    def accumulate_gradient(self) -> None:
        """`accumulate` > 1, after forward_backward() of one of the first k - 1 micro-batches: add its gradient to the
        accumulator (uz_tail_accumulate, one eager launch; the first of a group overwrites what the accumulator held)"""
        self._refuse_in_ema()
        if self._micro + 1 >= self.accumulate:
            raise RuntimeError(f"accumulate={self.accumulate}: {self._micro} micro-batches are accumulated, the next call is optimizer_step()")
        self.opt.accumulate_grad(self._micro == 0)
        self._micro += 1

    def __call__(self, x: Optional[torch.Tensor] = None, target: Optional[torch.Tensor] = None) -> torch.Tensor:
        """One call of the training loop.  With accumulate = k > 1 it is one MICRO-batch: calls 1 .. k-1 of a group run forward +
        backward and add the gradient to the accumulator, call k runs the optimizer tail on the mean of the k gradients;
        every call returns its own micro-batch's loss."""
        loss = self.forward_backward(x, target)
        if self._micro + 1 < self.accumulate:
            self.accumulate_gradient()
        else:
            self.optimizer_step()
        return loss

    # ------------------------------------------------------------------ the scheduled tail: EMA weights, state
    def _refuse_in_ema(self) -> None:
        if self._in_ema:
            raise RuntimeError("inside `with step.ema_weights():` the parameters ARE the averaged weights: no training step, "
                               "no state_dict() -- leave the context first")

    @contextlib.contextmanager
    def ema_weights(self):
        """``with step.ema_weights():`` -- evaluate, predict or save with the averaged weights.  The CONTENTS of the flat
        parameter buffer and of the EMA buffer are exchanged on entry and again on exit (uz_tail_swap, one launch each): no
        address moves, every captured graph stays valid, and since every forward begins with the pack cache's re-pack launch a
        following GraphedEval / GraphedPredict / model(x) / checkpoint.save_model_state sees the averaged weights.  Module
        BUFFERS (the BatchNorm running statistics) are shared, not averaged.  Training inside the context raises."""
        if self.ema_decay is None:
            raise RuntimeError("this GraphedStep keeps no averaged weights: build it with ema=<decay>")
        if self.opt is None:
            raise RuntimeError("ema_weights(): the averaged weights exist from the first training step on")
        if self._in_ema:
            raise RuntimeError("ema_weights() is not re-entrant")
        self.opt.swap_ema()
        self._in_ema = True
        try:
            yield self
        finally:
            self.opt.swap_ema()
            self._in_ema = False

    @property
    def lr_now(self) -> torch.Tensor:
        """the rate the last optimizer step used, a device scalar (scheduled tail: state[2], the schedule's value)"""
        if self._tail:
            return self.opt.last_lr()
        return torch.tensor(self.lr, dtype=torch.float32, device=self.opt.flat_p.device)

    def _param_names(self) -> List[str]:
        names = {id(p): n for n, p in self.model.named_parameters()}
        return [names[id(p)] for p in self.opt.params]

    def state_dict(self) -> dict:
        """What a resume needs beside the model's own state_dict (checkpoint.save_model_state): "step" (optimizer steps done),
        "lr" (the base rate), "micro" (micro-batches already accumulated towards the next step), "schedule" (the schedule's
        numbers, None without one; a record -- a resumed step keeps the schedule it was built with) and "state": by parameter
        name, detached clones of exp_avg, exp_avg_sq and, where the tail has them, ema and acc.  Reads the step counter: one
        host synchronize."""
        self._refuse_in_ema()
        if self.opt is None:
            raise RuntimeError("state_dict(): the optimizer state exists from the first training step on")
        opt = self.opt
        bufs = {"exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}
        for k in ("ema", "acc"):
            if getattr(opt, k, None) is not None:
                bufs[k] = getattr(opt, k)
        state = OrderedDict()
        for name, p, (a0, _) in zip(self._param_names(), opt.params, opt.spans):
            state[name] = {k: b[a0:a0 + p.numel()].view_as(p).detach().clone() for k, b in bufs.items()}
        return {"step": int(opt.step_count.item()), "lr": float(self.lr), "micro": self._micro,
                "schedule": self.schedule.numbers() if self.schedule is not None else None, "state": state}

    def load_state_dict(self, sd: dict) -> None:
        """Restore a state_dict() of a step built with the same arguments on the same model.  Before the first call the state
        is kept and applied at the end of the set-up (the flat buffers do not exist until then); parameter names or buffers
        that do not match raise."""
        for k in ("step", "lr", "micro", "state"):
            if k not in sd:
                raise KeyError(f"load_state_dict: no {k!r} in the state")
        if not 0 <= int(sd["micro"]) < self.accumulate:
            raise ValueError(f"load_state_dict: micro={sd['micro']} does not fit accumulate={self.accumulate}")
        if self.opt is None:
            self._pending_state = sd
        else:
            self._refuse_in_ema()
            self._apply_state(sd)

    def _apply_state(self, sd: dict) -> None:
        opt, names = self.opt, self._param_names()
        if set(names) != set(sd["state"]):
            odd = sorted(set(names) ^ set(sd["state"]))
            raise KeyError(f"load_state_dict: parameter names do not match: {odd[:6]}{' ...' if len(odd) > 6 else ''}")
        bufs = {"exp_avg": opt.exp_avg, "exp_avg_sq": opt.exp_avg_sq}
        for k in ("ema", "acc"):
            if getattr(opt, k, None) is not None:
                bufs[k] = getattr(opt, k)
        for name, p, (a0, _) in zip(names, opt.params, opt.spans):
            ent = sd["state"][name]
            if set(ent) != set(bufs):
                raise KeyError(f"load_state_dict: {name} holds {sorted(ent)}, this step's tail keeps {sorted(bufs)}")
            for k, b in bufs.items():
                if tuple(ent[k].shape) != tuple(p.shape):
                    raise ValueError(f"load_state_dict: {name}.{k} has shape {tuple(ent[k].shape)}, the parameter {tuple(p.shape)}")
                b[a0:a0 + p.numel()].view_as(p).copy_(ent[k])
        opt.step_count.fill_(float(sd["step"]))
        self.steps_done, self._micro = int(sd["step"]), int(sd["micro"])
        lr = float(sd["lr"])
        if self._tail:
            self.lr = lr
            opt.set_lr(lr)
        elif lr != opt.lr:
            self.lr = opt.lr = lr
            if self._g_opt is not None:          # the rate is an argument of the captured launches
                torch.cuda.synchronize()
                self._capture_opt()

    # ------------------------------------------------------------------ introspection
    @property
    def grad_norm(self) -> torch.Tensor:
        """total gradient norm the last optimizer step saw, before clipping (device scalar); with accumulate > 1 the norm of
        the MEAN gradient"""
        return self.opt.last_grad_norm()

    @property
    def augmented(self) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """(pictures, masks) the last step trained on: the augmentation's STATIC outputs (None without `augment`)"""
        g = self._cur
        return None if g is None or g.aug is None else (g.aug.out_image, g.aug.out_mask)

    @property
    def sampled(self) -> Optional[Tuple[torch.Tensor, torch.Tensor]]:
        """(pictures, masks) the sampler cut for the last step, before any augmentation: its STATIC outputs (None without
        `source`)"""
        g = self._cur
        return None if g is None or g.src is None else (g.src.out_image, g.src.out_mask)

    @property
    def coords(self) -> Optional[torch.Tensor]:
        """(B, 4) int32 [picture, y0, x0, plane or -1] of the last step's patches: the sampler's STATIC tensor (None without
        `source`)"""
        g = self._cur
        return None if g is None or g.src is None else g.src.coords

    @property
    def flat_grad(self) -> torch.Tensor:
        return self.opt.flat_g[:self.opt.n]

    def describe(self) -> str:
        """launch strategy in words (bench.py's `launch` field)"""
        k = len(self._cuts) - 1 if self._cuts else self.n_phases
        tail = []
        if self.schedule is not None:
            tail.append(f"{self.schedule.kind} schedule")
        if self.ema_decay is not None:
            tail.append("EMA")
        if self.accumulate > 1:
            tail.append(f"mean of {self.accumulate} accumulated gradients")
        opt = f"hipGraph({'+'.join(['clip', 'AdamW'] + tail)} on flat buffers, 3 launches)"
        crit = "" if self._fused_loss else "hipGraph(fwd) + eager criterion + "
        head = [name for name, opt_in in (("PatchSampler", self.source), ("GpuAugment", self.augment)) if opt_in is not None]
        if head:
            crit = " + ".join(head) + " at the head of the first hipGraph + " + crit
        if not self.distributed:
            return f"{crit}hipGraph({'fwd+' if self._fused_loss else ''}bwd) + {opt}"
        mb = [round((a1 - a0) * 4 / 2 ** 20, 1) for a0, a1 in self._spans]
        if self.comm_dtype == torch.bfloat16:
            opt = "gradient exchange in bf16 (all-to-all, fp32 sum on arrival, all-gather) + " + opt
        if self.comm == "tail":
            return (f"{crit}{k} hipGraphs ({'fwd + ' if self._fused_loss else ''}backward phases), then ONE RCCL all-reduce of "
                    f"{round(sum(mb), 1)} MB + {opt}")
        return (f"{crit}{k} hipGraphs ({'fwd + ' if self._fused_loss else ''}backward phases) with async RCCL "
                f"all-reduce of {mb} MB overlapped with the next phase + {opt}")
