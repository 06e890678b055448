"""GPU: unet_zoo_amd.GraphedEval -- the reference's evaluation pass (validate_one_epoch, unet_zoo/utils/training_loop.py:147-180:
model.eval(), torch.no_grad(), forward, loss, Dice) replayed from one hipGraph per input shape -- against the same pass
launched eagerly, with and without the eval-mode BatchNorm folded into the convolution epilogues (Engine.fold_bn_eval).

fold_bn=False: bit for bit in both run dtypes.  fold_bn=True: bit for bit in fp32 (both routes apply the same fmaf to the
same fp32 value); in bf16 the activations are rounded once instead of twice, so the logits are held to the bound
tests/test_bf16_rounded_oracle_gpu.py sets against the oracle that rounds where the two-launch engine stores
(oracle/torch_ref.set_storage_rounding), and the Dice -- a count of thresholded logits -- to equality, after checking on
the CPU that the oracle has no logit inside the rounding margin around zero for the seeds used, in all four models."""
import pytest
import torch

pytestmark = pytest.mark.gpu

import unet_zoo_amd
from oracle import torch_ref
from storage_move import move_two_weights, twin_of  # tests/storage_move.py
from unet_zoo_amd.engine import Engine
from unet_zoo_amd.loss import loss_and_dice

DEV = "cuda"
MODELS = {"unet": {}, "attention_unet": {}, "nested_unet": {"deep_supervision": True}, "u2net": {}}
ORACLE = {"unet": torch_ref.unet_forward, "attention_unet": torch_ref.attention_unet_forward,
          "nested_unet": torch_ref.nested_unet_forward, "u2net": torch_ref.u2net_forward}
# logits rms bound of the folded bf16 route against the storage-rounded oracle, relative to the logit norm
LOGIT_BOUND = 1e-2


def _make(name, dtype, **extra):
    """the model of the existing goldens (seed 0) with BatchNorm statistics and affine parameters moved off their initial
    0 / 1, so that the folded (scale, shift) are not the identity; returns (eval model on the GPU, its CPU state dict)"""
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model(name, in_channels=extra.pop("in_channels", 3), num_classes=1, **MODELS.get(name, {}), **extra)
    m.run_dtype = dtype
    g = torch.Generator().manual_seed(4)
    for mod in m.modules():
        if isinstance(mod, torch.nn.BatchNorm2d):
            C = mod.num_features
            mod.running_mean.copy_(0.1 * torch.randn(C, generator=g))
            mod.running_var.copy_(0.5 + torch.rand(C, generator=g))
            with torch.no_grad():
                mod.weight.copy_(0.5 + torch.rand(C, generator=g))
                mod.bias.copy_(0.1 * torch.randn(C, generator=g))
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return m.to(DEV).eval(), sd


def _batch(H=64, W=64, seed=1, C=3):
    x, t = torch_ref.synthetic_batch(2, C, H, W, seed=seed)
    return x.to(DEV), t.to(DEV)


def _flat(outputs):
    if isinstance(outputs, dict):
        return list(outputs.values())
    if isinstance(outputs, (list, tuple)):
        return list(outputs)
    return [outputs]


def _main(outputs):     # the output whose Dice loss_and_dice reports
    if isinstance(outputs, dict):
        return next(iter(outputs.values()))
    if isinstance(outputs, (list, tuple)):
        return outputs[-1]
    return outputs


def _eager(m, x, t):
    with torch.no_grad():
        out = m(x)
        loss, dice = loss_and_dice(out, t)
    torch.cuda.synchronize()
    return [o.clone() for o in _flat(out)], loss.clone(), dice.clone()


def _buffers(m):
    return {k: v.clone() for k, v in m.state_dict().items() if k not in dict(m.named_parameters())}


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(p, q) for p, q in zip(a, b))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
@pytest.mark.parametrize("name", list(MODELS))
def test_unfolded_replay_equals_eager_eval_bitwise(name, dtype):
    m, _ = _make(name, dtype)
    x, t = _batch()
    outs, loss, dice = _eager(m, x, t)
    buf0 = _buffers(m)
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice", fold_bn=False)
    l1, d1 = ev(x, t)
    torch.cuda.synchronize()
    assert l1.dim() == 0 and d1.dim() == 0 and l1.is_cuda
    assert type(ev.outputs) is type(m.wrap_outputs(tuple(outs)))
    first = [o.clone() for o in _flat(ev.outputs)]
    assert _same(first, outs) and torch.equal(l1, loss) and torch.equal(d1, dice)
    l1c = l1.clone()
    l2, d2 = ev(x, t)
    torch.cuda.synchronize()
    assert _same(_flat(ev.outputs), first) and torch.equal(l2, l1c) and torch.equal(d2, dice)
    assert ev.folded_layers == 0
    buf1 = _buffers(m)
    assert all(torch.equal(buf0[k], buf1[k]) for k in buf0)


@pytest.mark.parametrize("name", list(MODELS))
def test_folded_fp32_equals_eager_eval_bitwise(name):
    m, _ = _make(name, torch.float32)
    x, t = _batch()
    outs, loss, dice = _eager(m, x, t)
    buf0 = _buffers(m)
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice", fold_bn=True)
    l1, d1 = ev(x, t)
    torch.cuda.synchronize()
    assert ev.folded_layers > 0, "nothing took the one-launch route"
    if name == "unet":
        # 18 Conv -> BN -> ReLU layers: the 4 pooled ones stay on two launches, and so does the first one in fp32 (its
        # im2col product is a 1x1 problem of the LDS-DMA GEMM, which has no output activation)
        assert (ev.folded_layers, ev.unfolded_layers) == (13, 5)
    assert _same(_flat(ev.outputs), outs) and torch.equal(l1, loss) and torch.equal(d1, dice)
    ev(x, t)
    torch.cuda.synchronize()
    assert _same(_flat(ev.outputs), outs)
    buf1 = _buffers(m)
    assert all(torch.equal(buf0[k], buf1[k]) for k in buf0)
    assert Engine.fold_bn_eval is False          # the switch is the object's own: eager forwards stay as they were


@pytest.mark.parametrize("name", list(MODELS))
def test_folded_bf16_stays_within_the_rounded_oracle_bound(name):
    m, sd = _make(name, torch.bfloat16)
    x, t = _batch()
    torch_ref.set_storage_rounding(torch.bfloat16)
    try:
        with torch.no_grad():
            ref = _main(ORACLE[name](sd, x.cpu(), False))
    finally:
        torch_ref.set_storage_rounding(None)
    outs, loss, dice = _eager(m, x, t)          # the two-launch engine
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice", fold_bn=True)
    l1, d1 = ev(x, t)
    torch.cuda.synchronize()
    got = _main(ev.outputs).float().cpu()
    two = _main(m.wrap_outputs(tuple(outs))).float().cpu()
    e_fold = ((got - ref).norm() / ref.norm()).item()
    e_two = ((two - ref).norm() / ref.norm()).item()
    print(f"{name}: logits rms vs storage-rounded oracle: folded {e_fold:.3e}, two-launch {e_two:.3e}; folded layers "
          f"{ev.folded_layers}, unfolded {ev.unfolded_layers}; loss {l1.item():.6f} vs {loss.item():.6f}")
    assert ev.folded_layers > 0
    if name == "unet":
        # 18 Conv -> BN -> ReLU layers; the 4 pooled ones stay on two launches, and so does 512 -> 256 at 16 x 16: the
        # library plans it split over K with a workspace (conv3x3_pp256w16_bf16_splitk), a form whose result is rounded by
        # the reduce pass and which uz_conv_igemm_bnact leaves to the two-launch route.  (The issue counted 14 of 18: it
        # excludes the split-K forms and overlooked that this layer is one.)  A silent fallback of any other layer fails here.
        assert (ev.folded_layers, ev.unfolded_layers) == (13, 5)
    # the bound the issue names, for every model: 1e-2 of the logit norm against the storage-rounded oracle (unet's row in
    # tests/test_bf16_rounded_oracle_gpu.py; stricter than that file's rows for attention_unet and nested_unet, which hold
    # a TRAINING step -- batch statistics over 32 ... 8192 samples -- where this is an eval forward on fixed statistics)
    assert e_fold <= LOGIT_BOUND
    # Dice counts thresholded logits.  A logit whose oracle value is further from zero than the margin of
    # tests/test_bf16_rounded_oracle_gpu.py (4 x bound x max |logit|) cannot change sign within the bound; the BatchNorm
    # perturbation seed of _make() was chosen so that NO oracle logit lies inside it for any of the four models (on the
    # CPU: min |logit| 0.080 / 0.041 / 0.159 / 0.019 against margins 0.0064 / 0.0030 / 0.0079 / 0.0074), so the mask and
    # with it the Dice must be the eager route's exactly
    margin = 4 * LOGIT_BOUND * ref.abs().max()
    assert (ref.abs() > margin).all(), "an oracle logit inside the margin: pick another seed"
    assert torch.equal(got > 0, ref > 0) and torch.equal(two > 0, ref > 0)
    print(f"{name}: dice folded {d1.item():.6f}, eager {dice.item():.6f}; min |oracle logit| {ref.abs().min().item():.4f}, "
          f"margin {margin.item():.4f}")
    assert torch.equal(d1, dice)
    assert abs(l1.item() - loss.item()) < 5e-3


def test_evaluate_is_the_mean_over_batches_of_two_shapes():
    m, _ = _make("unet", torch.float32)
    batches = [_batch(64, 64, seed=1), _batch(48, 80, seed=5)]
    want = [_eager(m, x, t) for x, t in batches]
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice", fold_bn=True)
    loader = [(x.cpu(), t.cpu(), "name") for x, t in batches]      # host tensors, (img, mask, _) as the reference's loader
    ml, md = ev.evaluate(loader)
    assert len(ev._graphs) == 2
    assert ml == (want[0][1].double() + want[1][1].double()).item() / 2
    assert md == (want[0][2].double() + want[1][2].double()).item() / 2
    assert ev.evaluate(loader) == (ml, md) and len(ev._graphs) == 2
    # a callable criterion runs eagerly on the static outputs
    ev2 = unet_zoo_amd.GraphedEval(m, lambda out, tt: torch.nn.functional.binary_cross_entropy_with_logits(out, tt), fold_bn=True)
    l2, d2 = ev2(*batches[0])
    assert torch.allclose(l2, want[0][1], rtol=1e-6) and torch.equal(d2, want[0][2])


def test_an_optimizer_step_between_two_calls_is_seen():
    m, _ = _make("unet", torch.float32)
    x, t = _batch()
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice", fold_bn=True)
    ev(x, t)
    torch.cuda.synchronize()
    out0 = _main(ev.outputs).clone()
    m.train()
    step = unet_zoo_amd.GraphedStep(m, "bce_dice", lr=1e-2)
    step(x, t)                      # its first call gathers the parameters into one flat buffer: their storage moves
    m.eval()
    outs, loss, dice = _eager(m, x, t)
    l1, d1 = ev(x, t)
    torch.cuda.synchronize()
    assert not torch.equal(_main(ev.outputs), out0)
    assert _same(_flat(ev.outputs), outs) and torch.equal(l1, loss) and torch.equal(d1, dice)
    # a second step moves no storage: the SAME graph is replayed and re-packs the weights it reads
    g = next(iter(ev._graphs.values()))
    m.train()
    step(x, t)
    m.eval()
    outs2, loss2, _ = _eager(m, x, t)
    l2, _ = ev(x, t)
    torch.cuda.synchronize()
    assert next(iter(ev._graphs.values())) is g
    assert not _same(outs2, outs)
    assert _same(_flat(ev.outputs), outs2) and torch.equal(l2, loss2)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_a_parameter_on_new_storage_is_read_there(dtype):
    """storage that moves without GraphedStep: the new capture must read the new addresses (tests/storage_move.py)"""
    m, _ = _make("unet", dtype)
    x, t = _batch()
    with torch.no_grad():                     # the logits straddle zero, so that the Dice (a count of their signs) can move
        head_bias = [p for n, p in m.named_parameters() if n.endswith("bias") and p.numel() == 1][-1]
        head_bias -= _main(m(x)).float().median()
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice")
    l0, d0 = ev(x, t)
    torch.cuda.synchronize()
    out0, l0, d0 = _main(ev.outputs).clone(), l0.clone(), d0.clone()
    kept = move_two_weights(m)
    outs, loss, dice = _eager(twin_of(m, lambda: _make("unet", dtype)[0]), x, t)
    l1, d1 = ev(x, t)
    torch.cuda.synchronize()
    print(f"loss {l0.item():.6f} -> {l1.item():.6f} (eager {loss.item():.6f}), dice {d0.item():.6f} -> {d1.item():.6f} (eager {dice.item():.6f})")
    assert _same(_flat(ev.outputs), outs) and torch.equal(l1, loss) and torch.equal(d1, dice)
    assert not torch.equal(_main(ev.outputs), out0) and not torch.equal(l1, l0) and not torch.equal(d1, d0)
    assert len(ev._graphs) == 1 and len(kept) == 2
    # ... and so does the moved model's own eager forward from now on
    outs2, loss2, dice2 = _eager(m, x, t)
    assert _same(outs2, outs) and torch.equal(loss2, loss) and torch.equal(dice2, dice)


def test_vnet_keeps_its_reference_semantics():
    """vnet's normalisation uses batch statistics and updates its running statistics in eval mode too (the reference's
    ContBatchNorm): once per call through GraphedEval as well, and nothing in it is folded"""
    torch.manual_seed(0)
    m = unet_zoo_amd.create_model("vnet", in_channels=1, num_classes=1)
    m.run_dtype = torch.float32
    m = m.to(DEV).eval()
    x, t = torch_ref.synthetic_batch(2, 1, 32, 32, seed=2)
    x, t = x.to(DEV), t.to(DEV)
    before = {k: v.clone() for k, v in m.state_dict().items()}
    with torch.no_grad():
        want = m(x).clone()
    once = {k: v.clone() for k, v in m.state_dict().items()}
    m.load_state_dict(before)
    ev = unet_zoo_amd.GraphedEval(m, "bce_dice", fold_bn=True)
    ev(x, t)
    torch.cuda.synchronize()
    assert ev.folded_layers == 0
    assert torch.equal(ev.outputs, want)
    after = m.state_dict()
    moved = [k for k in before if k.endswith("running_mean") and not torch.equal(before[k], after[k])]
    assert moved, "vnet's running statistics did not move"
    assert all(torch.equal(after[k], once[k]) for k in before)      # exactly one forward's update


def test_train_mode_and_cpu_models_are_refused():
    m, _ = _make("unet", torch.float32)
    x, t = _batch()
    ev = unet_zoo_amd.GraphedEval(m.train(), "bce_dice")
    with pytest.raises(RuntimeError, match="eval"):
        ev(x, t)
    with pytest.raises(RuntimeError, match="eval"):
        ev.evaluate([(x, t)])
