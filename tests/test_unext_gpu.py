"""GPU: UNeXt / UNeXt-S on the HIP engine against the reference's golden vectors (tests/golden/unext_*: seed-0 models,
B = 2 at 64 x 64, UNeXt-S at a non-square 96 x 160), the bf16 run mode against the fp32 one, the graphed step against
the eager one, and run-to-run determinism."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import unet_zoo_amd
from oracle import torch_ref
from unet_zoo_amd.loss import loss_and_dice
from unet_zoo_amd.optim import FlatClipAdamW

DEV = "cuda"
GRAD_SAMPLES = {
    "unext": ("patch_embed1.proj.weight", "block1.0.attn.sr.weight", "block2.1.attn.kv.weight",
              "block3.5.mlp.dwconv.dwconv.weight", "decoder_level1.weight", "final_conv.weight"),
    "unext_s": ("patch_embed1.proj.weight", "block1.0.attn.q.weight", "block3.1.attn.proj.weight",
                "block2.0.mlp.fc1.weight", "decoder_level3.weight", "final_conv.bias"),
}


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def _golden(golden_dir, tag):
    with open(os.path.join(golden_dir, tag + ".json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(golden_dir, tag + ".npz"))


def _model(name, size, dtype=torch.float32):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=3, num_classes=1, image_size=size)
    m.run_dtype = dtype
    return m.to(DEV).train()


@pytest.mark.parametrize("name", ["unext", "unext_s"])
def test_fp32_step_matches_reference_golden(golden_dir, name):
    meta, arr = _golden(golden_dir, f"{name}_b2_64")
    x, mask = torch_ref.synthetic_batch(2, 3, 64, 64, seed=1)
    m = _model(name, 64)
    logits = m(x.to(DEV))
    loss = F.binary_cross_entropy_with_logits(logits, mask.to(DEV))
    loss.backward()
    ref = torch.from_numpy(arr["train_logits"])
    got = logits.detach().cpu()
    assert got.shape == ref.shape
    assert (got - ref).abs().max() <= 1e-3 * ref.abs().max()
    sure = ref.abs() > 1e-4 * ref.abs().max()
    assert torch.equal((got > 0)[sure], (ref > 0)[sure])
    assert abs(loss.item() - meta["loss"]) < 1e-5
    named = dict(m.named_parameters())
    assert {n for n, p in named.items() if p.grad is not None} == set(meta["grad_l2"])
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in named.values() if p.grad is not None)).item()
    assert abs(gn - meta["global_grad_norm"]) < 3e-3 * meta["global_grad_norm"]
    for n, rn in meta["grad_l2"].items():
        g = named[n].grad
        assert abs(g.double().norm().item() - rn) <= 2e-2 * rn + 1e-5 * meta["global_grad_norm"], (n, g.norm().item(), rn)
    for n in GRAD_SAMPLES[name]:
        gv = named[n].grad.flatten().cpu()[arr["gidx/" + n]].numpy()
        np.testing.assert_allclose(gv, arr["gval/" + n], rtol=5e-2, atol=2e-3 * np.abs(arr["gval/" + n]).max())
    m.eval()
    with torch.no_grad():
        ev = m(x.to(DEV)).cpu()
    evr = torch.from_numpy(arr["eval_logits"])
    assert (ev - evr).abs().max() <= 1e-3 * evr.abs().max()


@pytest.mark.parametrize("tag,H,W", [("unext_s_b1_100", 100, 100), ("unext_s_b1_96x160", 96, 160)])
def test_odd_and_non_square_inputs_match_reference_golden(golden_dir, tag, H, W):
    """100 x 100: token maps 25 / 13 / 7, which the reduction convolutions (r = 8 / 4 / 2) crop to 3 x 3 like Conv2d;
    96 x 160: a non-square map that every r divides"""
    meta, arr = _golden(golden_dir, tag)
    x, mask = torch_ref.synthetic_batch(1, 3, H, W, seed=1)
    m = _model("unext_s", H)
    logits = m(x.to(DEV))
    assert tuple(logits.shape) == (1, 1, H, W)
    loss = F.binary_cross_entropy_with_logits(logits, mask.to(DEV))
    loss.backward()
    idx = arr["logit_idx"]
    got = logits.detach().cpu().flatten()[idx]
    ref = torch.from_numpy(arr["train_logits_sampled"])
    assert (got - ref).abs().max() <= 1e-3 * ref.abs().max()
    assert abs(loss.item() - meta["loss"]) < 1e-5
    named = dict(m.named_parameters())
    assert {n for n, p in named.items() if p.grad is not None} == set(meta["grad_l2"])
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in named.values() if p.grad is not None)).item()
    assert abs(gn - meta["global_grad_norm"]) < 3e-3 * meta["global_grad_norm"]
    for n, rn in meta["grad_l2"].items():
        g = named[n].grad
        assert abs(g.double().norm().item() - rn) <= 2e-2 * rn + 1e-5 * meta["global_grad_norm"], (n, g.norm().item(), rn)
    m.eval()
    with torch.no_grad():
        ev = m(x.to(DEV)).cpu().flatten()[idx]
    evr = torch.from_numpy(arr["eval_logits_sampled"])
    assert (ev - evr).abs().max() <= 1e-3 * evr.abs().max()


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("H,W,r", [(25, 25, 8), (13, 7, 4), (7, 9, 2), (16, 24, 8)])
def test_space_to_depth_crops_like_conv2d(dt, H, W, r):
    """The reduction convolution's gather on a map r does not divide: the bottom / right border is not read, and the
    inverse (its input gradient) writes zeros there."""
    from unet_zoo_amd import ops
    from unet_zoo_amd.ops import act_from_nchw
    g = torch.Generator().manual_seed(H * 100 + W)
    N, C = 2, 16
    Ho, Wo = H // r, W // r
    x = torch.randn(N, C, H, W, generator=g).to(dt)
    xa = act_from_nchw(x.float().to(DEV), dt)
    cols = ops.new_act(N, Ho, Wo, r * r * C, dt, DEV)
    ops.space_to_depth(xa, cols, r)
    # cols[n, ho, wo, (ty*r + tx)*C + c] = x[n, c, ho*r + ty, wo*r + tx]
    want = x[:, :, :Ho * r, :Wo * r].reshape(N, C, Ho, r, Wo, r).permute(0, 2, 4, 3, 5, 1).reshape(N * Ho * Wo, r * r * C)
    assert torch.equal(cols.buf.cpu(), want)
    back = ops.new_act(N, H, W, C, dt, DEV)
    back.buf.fill_(7)
    ops.space_to_depth(cols, back, r, inverse=True)
    full = torch.zeros_like(x)
    full[:, :, :Ho * r, :Wo * r] = x[:, :, :Ho * r, :Wo * r]
    assert torch.equal(back.buf.cpu(), full.permute(0, 2, 3, 1).reshape(N * H * W, C))


@pytest.mark.parametrize("name", ["unext", "unext_s"])
def test_bf16_step_against_the_fp32_engine(name):
    x, mask = torch_ref.synthetic_batch(2, 3, 128, 128, seed=5)
    xs, ms = x.to(DEV), mask.to(DEV)
    runs = []
    for dt in (torch.float32, torch.bfloat16):
        m = _model(name, 128, dt)
        logits = m(xs)
        F.binary_cross_entropy_with_logits(logits, ms).backward()
        runs.append((logits.detach().float().cpu(), {n: p.grad.detach().float().cpu() for n, p in m.named_parameters()}))
    (l32, g32), (l16, g16) = runs
    assert relerr(l16, l32) < 6e-2
    a = torch.cat([g16[n].flatten() for n in g32])
    b = torch.cat([g32[n].flatten() for n in g32])
    assert F.cosine_similarity(a.double(), b.double(), dim=0).item() >= 0.9


def test_two_identical_steps_give_identical_gradients():
    x, mask = torch_ref.synthetic_batch(2, 3, 64, 64, seed=3)
    grads = []
    for _ in range(2):
        m = _model("unext", 64, torch.bfloat16)
        F.binary_cross_entropy_with_logits(m(x.to(DEV)), mask.to(DEV)).backward()
        grads.append([p.grad.clone() for p in m.parameters()])
    assert all(torch.equal(a, b) for a, b in zip(*grads))


def test_graphed_step_equals_eager_step_bitwise():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 64, 64, generator=g).cuda()
    t = (torch.rand(2, 1, 64, 64, generator=g) > 0.5).float().cuda()
    m1 = _model("unext_s", 64, torch.bfloat16)
    gs = unet_zoo_amd.GraphedStep(m1, "bce_dice", lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    g_losses, g_norms = [], []
    for _ in range(3):
        loss = gs(x, t)
        torch.cuda.synchronize()
        g_losses.append(loss.item())
        g_norms.append(gs.grad_norm.item())
    m2 = _model("unext_s", 64, torch.bfloat16)
    n1 = {id(p): n for n, p in m1.named_parameters()}
    p2 = dict(m2.named_parameters())
    opt = FlatClipAdamW([p2[n1[id(p)]] for p in gs.opt.params], lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    m2._pack_cache.repoint()
    m2.grads_in_place = True
    e_losses, e_norms = [], []
    for _ in range(3):
        loss, _dice = loss_and_dice(m2(x), t)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        e_losses.append(loss.item())
        e_norms.append(opt.last_grad_norm().item())
    assert g_losses == e_losses and g_norms == e_norms
    assert torch.equal(gs.opt.flat_p, opt.flat_p)
