"""GPU: swin_unet_v2 with windows above 8x8 (window_size 9 .. 16: 81 .. 256 tokens per window, the wide kernels of uz_winattn.hip).

1. fp32 train step + eval at 128 / window 16 and 96 / window 12 against the reference's goldens
   (tools/gen_golden_swin_wide.py), with the bounds of test_swin_gpu.py::test_swin_fp32_step_matches_reference_golden.  The
   masks are compared where |ref| > 1e-3 max|ref| -- inside that band a run within the logit bound may flip a sign -- and the
   band may hold 0.5 % of the pixels at most (the reference's own logits: 58 of 32 768 and 36 of 18 432).
2. bf16 at 128 / window 16 against the oracle, with the bounds of test_swin_bf16_two_classes_against_oracle_and_trains, then
   8 AdamW steps.
3. GraphedStep at 128 / window 16 in bf16: three replayed steps equal three eager steps bit for bit.
4. window_size 17 is refused with a message that names the 16x16 limit; window_size 8 runs twice to the same bits.
5. The continuous position bias at N^2 = 65 536 and 20 736 offsets, forward and backward through the batched entry points,
   against autograd."""
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import unet_zoo_amd
from oracle import torch_ref
from unet_zoo_amd import _lib as L
from unet_zoo_amd import ops
from unet_zoo_amd.loss import loss_and_dice
from unet_zoo_amd.optim import FlatClipAdamW

DEV = "cuda"


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / (b.double().abs().max() + 1e-30)).item()


def _golden(golden_dir, tag):
    with open(os.path.join(golden_dir, tag + ".json")) as f:
        meta = json.load(f)
    return meta, np.load(os.path.join(golden_dir, tag + ".npz"))


def _swin(img, ws, dpr=0.0, dtype=torch.float32, K=1):
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("swin_unet_v2", image_size=img, in_channels=3, num_classes=K, window_size=ws,
                                  drop_path_rate=dpr)
    m.run_dtype = dtype
    return m


def _masks_equal_outside_the_band(got, ref):
    band = ref.abs() <= 1e-3 * ref.abs().max()
    share = band.float().mean().item()
    print(f"  mask band: {int(band.sum())} of {band.numel()} pixels ({100 * share:.3f} %)")
    assert share <= 0.005
    assert torch.equal((got > 0)[~band], (ref > 0)[~band])


@pytest.mark.parametrize("img,ws", [(128, 16), (96, 12)])
def test_swin_wide_fp32_step_matches_reference_golden(golden_dir, img, ws):
    meta, arr = _golden(golden_dir, f"swin_unet_v2_b2_{img}_ws{ws}")
    x, mask = torch_ref.synthetic_batch(2, 3, img, img, seed=1)
    m = _swin(img, ws).to(DEV).train()
    logits = m(x.to(DEV))
    loss = F.binary_cross_entropy_with_logits(logits, mask.to(DEV))
    loss.backward()
    ref = torch.from_numpy(arr["train_logits"])
    got = logits.detach().cpu()
    named = dict(m.named_parameters())
    gn = torch.sqrt(sum((p.grad.double() ** 2).sum() for p in named.values() if p.grad is not None)).item()
    print(f"  logits {relerr(got, ref):.3e} of max (bound 1e-3), loss {loss.item():.7f} vs {meta['loss']:.7f}, "
          f"gradient norm {gn:.6f} vs {meta['global_grad_norm']:.6f}")
    assert (got - ref).abs().max() <= 1e-3 * ref.abs().max()
    _masks_equal_outside_the_band(got, ref)
    assert abs(loss.item() - meta["loss"]) < 1e-5
    assert {n for n, p in named.items() if p.grad is None} == set(meta["unused_parameters"])
    assert abs(gn - meta["global_grad_norm"]) < 2e-3 * meta["global_grad_norm"]
    for name, rn in meta["grad_l2"].items():
        g = named[name].grad
        assert abs(g.double().norm().item() - rn) <= 1e-2 * rn + 1e-5 * meta["global_grad_norm"], (name, g.norm().item(), rn)
        idx = torch.from_numpy(arr["gidx/" + name]).to(DEV)
        np.testing.assert_allclose(g.flatten()[idx].cpu().numpy(), arr["gval/" + name], rtol=2e-2,
                                   atol=2e-5 * max(rn, 1e-3), err_msg=name)
    m.eval()
    with torch.no_grad():
        ev = m(x.to(DEV)).cpu()
    evr = torch.from_numpy(arr["eval_logits"])
    assert (ev - evr).abs().max() <= 1e-3 * evr.abs().max()
    _masks_equal_outside_the_band(ev, evr)


def test_swin_wide_bf16_against_oracle_and_trains():
    m = _swin(128, 16, dpr=0.0, dtype=torch.bfloat16)
    sd0 = {k: v.clone() for k, v in m.state_dict().items()}
    m = m.to(DEV).train()
    x, mask = torch_ref.synthetic_batch(2, 3, 128, 128, seed=9)
    out = m(x.to(DEV))
    loss = F.binary_cross_entropy_with_logits(out, mask.to(DEV))
    loss.backward()
    cfg = torch_ref.swin_config(sd0, 128, window_size=16, drop_path_rate=0.0)
    rl, rloss, rg, _ = torch_ref.train_step_reference("swin_unet_v2", sd0, x, mask, cfg=cfg)
    got = out.detach().float().cpu()
    named = dict(m.named_parameters())
    gflat = torch.cat([named[n].grad.flatten().cpu() for n in rg])
    rflat = torch.cat([rg[n].flatten() for n in rg])
    cos = F.cosine_similarity(gflat.double(), rflat.double(), dim=0).item()
    print(f"  logits max |d| {(got - rl).abs().max().item():.4f} (max |ref| {rl.abs().max().item():.4f}), "
          f"loss {loss.item():.5f} vs {rloss.item():.5f}, gradient cosine {cos:.5f}")
    assert (got - rl).abs().max() <= 0.05 * rl.abs().max() + 0.02
    assert abs(loss.item() - rloss.item()) < 2e-2
    assert cos > 0.98, cos
    opt = torch.optim.AdamW([p for p in m.parameters()], lr=2e-4)
    xs, ms = x.to(DEV), mask.to(DEV)
    losses = []
    for _ in range(8):
        opt.zero_grad()
        l = F.binary_cross_entropy_with_logits(m(xs), ms)
        l.backward()
        opt.step()
        losses.append(l.item())
    assert all(np.isfinite(losses)) and losses[-1] < losses[0], losses


def test_swin_wide_replayed_step_equals_eager_step_bitwise():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 3, 128, 128, generator=g).cuda()
    t = (torch.rand(2, 1, 128, 128, generator=g) > 0.5).float().cuda()
    m1 = _swin(128, 16, dtype=torch.bfloat16).cuda().train()
    gs = unet_zoo_amd.GraphedStep(m1, "bce_dice", lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    g_losses, g_norms = [], []
    for _ in range(3):
        loss = gs(x, t)
        torch.cuda.synchronize()
        g_losses.append(loss.item())
        g_norms.append(gs.grad_norm.item())
    m2 = _swin(128, 16, dtype=torch.bfloat16).cuda().train()
    n1 = {id(p): n for n, p in m1.named_parameters()}
    p2 = dict(m2.named_parameters())
    opt = FlatClipAdamW([p2[n1[id(p)]] for p in gs.opt.params], lr=1e-3, weight_decay=1e-5, max_norm=1.0)
    m2._pack_cache.repoint()
    m2.grads_in_place = True
    e_losses, e_norms = [], []
    for _ in range(3):
        loss, dice = loss_and_dice(m2(x), t)
        loss.backward()
        opt.step()
        torch.cuda.synchronize()
        e_losses.append(loss.item())
        e_norms.append(opt.last_grad_norm().item())
    assert g_losses == e_losses, (g_losses, e_losses)
    assert g_norms == e_norms, (g_norms, e_norms)
    assert torch.equal(gs.opt.flat_p, opt.flat_p)
    assert all(l == l and 0.0 < l < 20.0 for l in g_losses)


def test_window_17_is_refused_and_window_8_is_unchanged():
    m = _swin(136, 17).to(DEV).eval()
    with pytest.raises(L.HipLibraryError, match="16x16"):
        with torch.no_grad():
            m(torch.zeros(1, 3, 136, 136, device=DEV))
    x, _ = torch_ref.synthetic_batch(2, 3, 64, 64, seed=1)
    outs = []
    for _ in range(2):
        m8 = _swin(64, 8).to(DEV).train()
        y = m8(x.to(DEV))
        y.sum().backward()
        outs.append((y.detach().clone(), m8.layers[0].blocks[1].attn.tau.grad.clone(),
                     m8.layers[0].blocks[1].attn.qkv.weight.grad.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("heads,N", [(3, 256), (6, 144)])
def test_continuous_position_bias_at_wide_window_sizes(heads, N):
    """R = N^2 = 65 536 / 20 736 offsets through uz_cpb_fwd_batched / uz_cpb_bwd_batched (512 / 162 row blocks of partial
    sums) against autograd in float64 on the same fp32 operands; tolerances of test_continuous_position_bias_mlp.  The
    offsets are the model's own table (log-spaced window offsets), the upstream gradient is random."""
    g = torch.Generator().manual_seed(47)
    R, ws = N * N, int(round(N ** 0.5))
    c = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing="ij")).flatten(1)
    rel = (c[:, :, None] - c[:, None, :]).permute(1, 2, 0).float()
    idx = (torch.sign(rel) * torch.log(1.0 + rel.abs())).reshape(R, 2).contiguous()
    w1 = torch.randn(256, 2, generator=g)
    b1 = torch.randn(256, generator=g) * 0.5
    w2 = torch.randn(heads, 256, generator=g) * 0.1
    b2 = torch.randn(heads, generator=g)
    G = torch.randn(heads, R, generator=g)
    p64 = [t.double().requires_grad_(True) for t in (w1, b1, w2, b2)]
    ref = F.linear(F.relu(F.linear(idx.double(), p64[0], p64[1])), p64[2], p64[3]).t()
    ref.backward(G.double())
    m = {k: t.to(DEV).contiguous() for k, t in (("idx", idx), ("w1", w1), ("b1", b1), ("w2", w2), ("b2", b2), ("G", G))}
    m["bias"] = torch.full((heads, R), float("nan"), device=DEV)
    for k, t in (("dw1", w1), ("db1", b1), ("dw2", w2), ("db2", b2)):
        m[k] = torch.full(t.shape, float("nan"), device=DEV)
    ops.cpb_fwd_batched([m])
    ops.cpb_bwd_batched([m])
    e = relerr(m["bias"].cpu(), ref.detach())
    print(f"  bias: {e:.3e} (tolerance 2e-6)")
    errs = {k: relerr(m[k].cpu(), p.grad) for k, p in zip(("dw1", "db1", "dw2", "db2"), p64)}
    print("  " + ", ".join(f"{k}: {v:.3e}" for k, v in errs.items()) + " (tolerance 1e-5)")
    assert e < 2e-6
    for k, v in errs.items():
        assert v < 1e-5, (k, v)
