"""GPU: GraphedStep with the scheduled tail (schedule= / ema= / accumulate=) -- against the default step where they must agree
bit for bit, against a twin driven eagerly by FlatClipAdamW for what is new.  unet, B = 2, 3 x 64 x 64, bf16, built as in
tests/test_step_gpu.py."""
import os

import numpy as np
import pytest
import torch

import unet_zoo_amd
from unet_zoo_amd import GraphedStep, LrSchedule, checkpoint
from unet_zoo_amd.loss import loss_and_dice
from unet_zoo_amd.optim import FlatClipAdamW, FlatTail

pytestmark = pytest.mark.gpu

LR = 1e-3
LR32 = float(np.float32(LR))
KW = dict(lr=LR, weight_decay=1e-5, max_norm=1.0)
COSINE = dict(total_steps=6, warmup_steps=2, min_lr=1e-5, warmup_start=0.1)


def _make():
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=1)
    m.run_dtype = torch.bfloat16
    return m.cuda().train()


def _batch(seed=1, b=2, size=64):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(b, 3, size, size, generator=g).cuda(), (torch.rand(b, 1, size, size, generator=g) > 0.5).float().cuda())


def _eager_twin(gs):
    """a second model with FlatClipAdamW over the parameters in gs's flat order, its backward writing in place"""
    m2 = _make()
    names = {id(p): n for n, p in gs.model.named_parameters()}
    p2 = dict(m2.named_parameters())
    opt = FlatClipAdamW([p2[names[id(p)]] for p in gs.opt.params], **KW)
    m2._pack_cache.repoint()
    m2.grads_in_place = True
    return m2, opt


def test_constant_schedule_is_the_default_step_bitwise():
    x, t = _batch()
    a = GraphedStep(_make(), "bce_dice", schedule=LrSchedule.constant(), **KW)
    b = GraphedStep(_make(), "bce_dice", **KW)
    for i in range(3):
        la, lb = a(x, t), b(x, t)
        torch.cuda.synchronize()
        assert la.item() == lb.item() and a.dice.item() == b.dice.item(), i
        assert a.grad_norm.item() == b.grad_norm.item(), i
        assert torch.equal(a.opt.flat_p, b.opt.flat_p), i
    assert type(a.opt) is FlatTail and type(b.opt) is FlatClipAdamW
    assert a.steps_done == b.steps_done == 3 and a.lr_now.item() == b.lr_now.item() == LR32
    assert b.describe().endswith("hipGraph(clip+AdamW on flat buffers, 3 launches)")
    assert a.describe().endswith("hipGraph(clip+AdamW+constant schedule on flat buffers, 3 launches)")


def test_set_lr_is_a_device_fill_and_keeps_the_graph():
    x, t = _batch()
    gs = GraphedStep(_make(), "bce_dice", schedule=LrSchedule.constant(), **KW)
    gs(x, t)
    graph = gs._g_opt
    gs.set_lr(0.0)
    assert gs._g_opt is graph
    before = gs.opt.flat_p.clone()
    gs(x, t)
    torch.cuda.synchronize()
    assert torch.equal(before, gs.opt.flat_p) and gs.lr_now.item() == 0.0      # the update and the decay both carry the rate
    gs.set_lr(LR)
    gs(x, t)
    assert gs._g_opt is graph and gs.lr_now.item() == LR32 and not torch.equal(before, gs.opt.flat_p)


def test_cosine_with_warmup_follows_lr_at():
    x, t = _batch()
    sched = LrSchedule.cosine(**COSINE)
    gs = GraphedStep(_make(), "bce_dice", schedule=sched, **KW)
    trace = []
    for _ in range(6):
        gs(x, t)
        trace.append(gs.lr_now.item())
    m2, opt = _eager_twin(gs)
    for i in range(6):
        want = sched.lr_at(i, LR32)
        assert abs(trace[i] - want) <= 1e-6 * want, (i, trace[i], want)
        opt.lr = want
        loss, _ = loss_and_dice(m2(x), t)
        loss.backward()
        opt.step()
    assert trace[0] == pytest.approx(0.1 * LR) and trace[2] == LR32 and trace[5] < trace[4] < trace[3] < trace[2]
    rel = ((gs.opt.flat_p - opt.flat_p).abs().max() / gs.opt.flat_p.abs().max()).item()
    print(f"cosine: lr trace {trace}; flat_p vs the eager twin: {rel:.2e} of the largest parameter")
    assert rel < 1e-5, rel
    assert "cosine schedule" in gs.describe()


def test_ema_context_swaps_the_averaged_weights_in_and_out():
    x, t = _batch()
    m = _make()
    gs = GraphedStep(m, "bce_dice", ema=0.9, **KW)
    with pytest.raises(RuntimeError):
        with gs.ema_weights():           # nothing to average before the first step
            pass
    for _ in range(4):
        gs(x, t)
    ema = {k: v["ema"] for k, v in gs.state_dict()["state"].items()}
    live = {k: p.detach().clone() for k, p in m.named_parameters()}
    ptrs = [p.data_ptr() for p in m.parameters()]
    assert any(not torch.equal(ema[k], live[k]) for k in ema)
    twin = _make()
    twin.load_state_dict(m.state_dict())                    # the buffers (BatchNorm running statistics) are shared, not averaged
    with torch.no_grad():
        for k, p in twin.named_parameters():
            p.copy_(ema[k])
    with gs.ema_weights():
        for k, p in m.named_parameters():
            assert torch.equal(p.detach(), ema[k]), k
        with pytest.raises(RuntimeError, match="ema_weights"):
            gs(x, t)
        m.eval()
        got, _ = unet_zoo_amd.GraphedEval(m, "bce_dice")(x, t)
        m.train()
        want, _ = unet_zoo_amd.GraphedEval(twin.eval(), "bce_dice")(x, t)
        assert got.item() == want.item()
    for k, p in m.named_parameters():
        assert torch.equal(p.detach(), live[k]), k
    assert [p.data_ptr() for p in m.parameters()] == ptrs
    gs(x, t)                                                  # and training goes on
    assert gs.steps_done == 5 and "EMA" in gs.describe()
    with pytest.raises(RuntimeError, match="ema="):
        with GraphedStep(_make(), "bce_dice", **KW).ema_weights():
            pass


def test_accumulate_two_micro_batches():
    (x1, t1), (x2, t2) = _batch(1), _batch(2)
    gs = GraphedStep(_make(), "bce_dice", accumulate=2, **KW)
    l1 = gs(x1, t1).item()
    assert gs.steps_done == 0 and gs._micro == 1
    before = gs.opt.flat_p.clone()
    l2 = gs(x2, t2).item()
    assert gs.steps_done == 1 and gs._micro == 0 and not torch.equal(before, gs.opt.flat_p)
    m2, opt = _eager_twin(gs)
    grads, losses = [], []
    for x, t in ((x1, t1), (x2, t2)):
        loss, _ = loss_and_dice(m2(x), t)
        loss.backward()
        grads.append(opt.flat_g.clone())
        losses.append(loss.item())
    opt.flat_g.copy_(((grads[0].double() + grads[1].double()) / 2).float())
    opt.step()
    assert [l1, l2] == losses                                   # every call returns its own micro-batch's loss
    ng, ne = gs.grad_norm.item(), opt.last_grad_norm().item()
    rel = ((gs.opt.flat_p - opt.flat_p).abs().max() / opt.flat_p.abs().max()).item()
    print(f"accumulate=2: norm {ng!r} vs {ne!r}; flat_p {rel:.2e} of the largest parameter")
    assert abs(ng - ne) <= 1e-6 * ne and rel < 1e-5
    for (k, a), (_, b) in zip(gs.model.named_buffers(), m2.named_buffers()):      # BatchNorm statistics advance per micro-batch
        assert torch.equal(a, b), k
    assert "mean of 2 accumulated gradients" in gs.describe()


def test_resume_mid_accumulation_is_bitwise(tmp_path):
    batches = [_batch(s) for s in range(1, 7)]
    args = dict(schedule=LrSchedule.cosine(**COSINE), ema=0.9, accumulate=2, **KW)
    whole = GraphedStep(_make(), "bce_dice", **args)
    for x, t in batches:
        whole(x, t)
    m1 = _make()
    first = GraphedStep(m1, "bce_dice", **args)
    for x, t in batches[:3]:
        first(x, t)
    sd = first.state_dict()
    assert (sd["step"], sd["micro"], sd["lr"]) == (1, 1, LR) and sd["schedule"]["kind"] == "cosine"
    assert set(sd["state"]) == {k for k, _ in m1.named_parameters()}
    assert all(set(v) == {"exp_avg", "exp_avg_sq", "ema", "acc"} for v in sd["state"].values())
    path = os.path.join(tmp_path, "model.pth")
    checkpoint.save_model_state(m1, path)
    torch.save(sd, os.path.join(tmp_path, "step.pth"))
    m2 = _make()
    with torch.no_grad():
        for p in m2.parameters():
            p.add_(1.0)                                        # whatever it held, the checkpoint replaces
    checkpoint.load_model_state(m2, path, "cuda")
    second = GraphedStep(m2.train(), "bce_dice", **args)
    second.load_state_dict(torch.load(os.path.join(tmp_path, "step.pth")))      # before its first call: kept until the set-up
    for x, t in batches[3:]:
        second(x, t)
    torch.cuda.synchronize()
    assert second.steps_done == whole.steps_done == 3 and second._micro == whole._micro == 0
    assert torch.equal(second.opt.flat_p, whole.opt.flat_p) and torch.equal(second.opt.ema, whole.opt.ema)
    assert torch.equal(second.opt.state, whole.opt.state)
    # after the first call too, and names that do not match raise
    second.load_state_dict(sd)
    assert second.steps_done == 1 and second._micro == 1 and second.opt.step_count.item() == 1.0
    bad = dict(sd, state={("x." + k): v for k, v in sd["state"].items()})
    with pytest.raises(KeyError, match="names"):
        second.load_state_dict(bad)
    with pytest.raises(KeyError, match="names"):
        fresh = GraphedStep(_make(), "bce_dice", **args)
        fresh.load_state_dict(bad)
        fresh(*batches[0])


def test_default_tail_has_a_state_too():
    x, t = _batch()
    whole = GraphedStep(_make(), "bce_dice", **KW)
    for _ in range(4):
        whole(x, t)
    m1 = _make()
    first = GraphedStep(m1, "bce_dice", **KW)
    for _ in range(2):
        first(x, t)
    sd = first.state_dict()
    assert (sd["step"], sd["micro"], sd["schedule"]) == (2, 0, None)
    assert all(set(v) == {"exp_avg", "exp_avg_sq"} for v in sd["state"].values())
    m2 = _make()
    m2.load_state_dict({k: v.detach().clone() for k, v in m1.state_dict().items()})
    second = GraphedStep(m2, "bce_dice", **KW)
    second.load_state_dict(sd)
    for _ in range(2):
        second(x, t)
    assert torch.equal(second.opt.flat_p, whole.opt.flat_p) and second.opt.step_count.item() == 4.0


@pytest.mark.parametrize("kw,err,arg", [
    (dict(accumulate=0), ValueError, "accumulate"),
    (dict(ema=1.5), ValueError, "ema"),
    (dict(schedule="cosine"), TypeError, "schedule"),
])
def test_refusals_name_the_argument(kw, err, arg):
    with pytest.raises(err, match=arg):
        GraphedStep(_make(), "bce_dice", **kw)
