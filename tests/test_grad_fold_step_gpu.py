"""GPU: whole training steps with Engine.fold_head_grad / Engine.fold_first_bn_bwd on and off: three GraphedStep steps of unet
(takes both routes) and of attention_unet (its first block is pooled: the first-layer route falls back) -- loss, outputs,
parameters, gradients and BatchNorm buffers bit for bit."""
import pytest
import torch

import unet_zoo_amd
from unet_zoo_amd.engine import Engine

pytestmark = pytest.mark.gpu


def _run(name, on):
    old = Engine.fold_head_grad, Engine.fold_first_bn_bwd
    Engine.fold_head_grad = Engine.fold_first_bn_bwd = on
    try:
        torch.manual_seed(0)
        m = unet_zoo_amd.create_model(name, in_channels=3, num_classes=1)
        m.run_dtype = torch.bfloat16
        m = m.cuda().train()
        g = torch.Generator().manual_seed(1)
        x = torch.randn(2, 3, 64, 64, generator=g).cuda()
        t = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().cuda()
        gs = unet_zoo_amd.GraphedStep(m, "bce_dice", lr=1e-3, weight_decay=1e-5, max_norm=1.0)
        losses = []
        for _ in range(3):
            losses.append(gs(x, t).item())
        torch.cuda.synchronize()
        names = {id(p): n for n, p in m.named_parameters()}
        order = [names[id(p)] for p in gs.opt.params]
        return (losses, gs.outputs.clone(), gs.opt.flat_p.clone(), gs.opt.flat_g.clone(), order,
                {k: b.clone() for k, b in m.named_buffers()})
    finally:
        Engine.fold_head_grad, Engine.fold_first_bn_bwd = old


@pytest.mark.parametrize("name", ["unet", "attention_unet"])
def test_steps_are_bitwise_the_same_with_and_without_the_folds(name):
    a, b = _run(name, True), _run(name, False)
    assert a[0] == b[0], (a[0], b[0])
    assert all(l == l and 0.0 < l < 20.0 for l in a[0])
    assert a[4] == b[4]
    assert torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])
    assert a[5].keys() == b[5].keys()
    for k in a[5]:
        assert torch.equal(a[5][k], b[5][k]), k


def test_unet_takes_both_folded_routes():
    """the switches route: with them on, a unet backward calls the two new entries (and not with them off)"""
    from unet_zoo_amd import ops
    seen = []
    real_head, real_first = ops.bn_relu_bwd_head, ops.conv_first_wgrad_bn
    ops.bn_relu_bwd_head = lambda *a, **k: (seen.append("head"), real_head(*a, **k))[1]
    ops.conv_first_wgrad_bn = lambda *a, **k: (seen.append("first"), real_first(*a, **k))[1]
    try:
        torch.manual_seed(0)
        m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=1)
        m.run_dtype = torch.bfloat16
        m = m.cuda().train()
        x = torch.randn(2, 3, 32, 32, device="cuda")
        m(x).sum().backward()
        assert sorted(seen) == ["first", "head"], seen
        del seen[:]
        Engine.fold_head_grad = Engine.fold_first_bn_bwd = False
        m(x).sum().backward()
        assert seen == []
    finally:
        Engine.fold_head_grad = Engine.fold_first_bn_bwd = True
        ops.bn_relu_bwd_head, ops.conv_first_wgrad_bn = real_head, real_first
