"""Generate the VNet goldens under tests/golden/ from the reference's own vnet.py (build machine only: the reference tree
is not on the GPU machines).  Uses oracle.gen_golden's loader, manifest writer, hash and index sampler unchanged.

    python tools/gen_golden_vnet.py

Writes vnet_manifest.json (seed 0, defaults), vnet_b2_64 (in_channels = 1) and vnet_c3_b2_64 (in_channels = 3: the residual
branch of the input stage goes through a 1x1 convolution the reference creates inside every forward).  The random draws of
the reference's forward are RECORDED -- the eight Dropout2d channel masks by forward hooks, the 1x1 convolution's weight and
bias by wrapping nn.Conv2d while the forward runs -- so that the engine can be fed the same ones (VNet.force_draws).  Each
json also holds `ref_fp32_vs_fp64`: the reference's own deviation between a float32 and a float64 run with the same draws,
the noise floor that the GPU tests' bounds are set against."""
import json
import os
import sys

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle.gen_golden import OUT, load_reference, sample_idx, sha, write_manifest  # noqa: E402
from oracle.torch_ref import synthetic_batch  # noqa: E402

BN_KEYS = ("in_tr.bn1", "down_tr256.ops.1.bn1", "out_tr.bn1")


class Draws:
    """record (masks=None) or replay the reference forward's random draws"""

    def __init__(self, model, masks=None, adapter=None):
        self.model, self.replay = model, masks is not None
        self.masks = list(masks) if masks is not None else []
        self.adapter = adapter
        self._i = 0

    def _hook(self, mod, inp, out):
        if not mod.training:
            return None
        if self.replay:
            m = self.masks[self._i]
            self._i += 1
            return inp[0] * (m.to(inp[0].dtype) * 2.0)[:, :, None, None]
        self.masks.append((out.detach().abs().amax((2, 3)) > 0).float())
        return None

    def __enter__(self):
        self._i = 0
        self.handles = [m.register_forward_hook(self._hook) for m in self.model.modules() if isinstance(m, nn.Dropout2d)]
        self._conv2d = nn.Conv2d
        outer = self

        def factory(*a, **k):
            conv = outer._conv2d(*a, **k)
            if outer.adapter is None:
                outer.adapter = (conv.weight.detach().clone(), conv.bias.detach().clone())
            else:
                conv = conv.to(outer.adapter_dtype)
                with torch.no_grad():
                    conv.weight.copy_(outer.adapter[0])
                    conv.bias.copy_(outer.adapter[1])
            return conv

        self.adapter_dtype = next(self.model.parameters()).dtype
        nn.Conv2d = factory
        return self

    def __exit__(self, *exc):
        nn.Conv2d = self._conv2d
        for h in self.handles:
            h.remove()


def step(model, x, mask, draws):
    model.train()
    model.zero_grad()
    with draws:
        logits = model(x)
    loss = F.binary_cross_entropy_with_logits(logits, mask.to(logits.dtype))
    loss.backward()
    named = [(n, p) for n, p in model.named_parameters() if p.grad is not None]
    gnorm = torch.sqrt(sum((p.grad.double() ** 2).sum() for _, p in named)).item()
    return logits.detach(), loss.item(), named, gnorm


def run_case(ref, cin, tag, full):
    torch.manual_seed(0)
    model = ref.VNet(in_channels=cin, num_classes=1)
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    x, mask = synthetic_batch(2, cin, 64, 64, seed=1)
    rec = Draws(model)
    logits, loss, named, gnorm = step(model, x, mask, rec)
    assert len(rec.masks) == 8, len(rec.masks)
    arrays = {f"mask/{i}": m.numpy() for i, m in enumerate(rec.masks)}
    if cin not in (1, 16):
        arrays["adapter/weight"], arrays["adapter/bias"] = rec.adapter[0].numpy(), rec.adapter[1].numpy()
    meta = {"model": "vnet", "in_channels": cin, "B": 2, "H": 64, "W": 64, "input_sha256": sha(x), "mask_sha256": sha(mask),
            "loss": loss, "global_grad_norm": gnorm, "grad_l2": {n: p.grad.double().norm().item() for n, p in named}}
    flat = logits.flatten()
    idx = sample_idx(flat.numel(), 4096)
    arrays["logit_idx"], arrays["train_logits_sampled"] = idx, flat[idx].numpy()
    if full:
        arrays["train_logits"] = logits.numpy()
        for n, p in named:
            gi = sample_idx(p.numel(), 64)
            arrays["gidx/" + n], arrays["gval/" + n] = gi, p.grad.flatten()[gi].numpy()
    sd = model.state_dict()
    for k in BN_KEYS:
        arrays["rm/" + k], arrays["rv/" + k] = sd[k + ".running_mean"].numpy().copy(), sd[k + ".running_var"].numpy().copy()
    assert all(int(v) == 0 for k, v in sd.items() if k.endswith("num_batches_tracked"))
    model.eval()
    with torch.no_grad(), Draws(model, rec.masks, rec.adapter):
        ev = model(x)
    arrays["eval_logits_sampled"] = ev.flatten()[idx].numpy()
    if full:
        arrays["eval_logits"] = ev.numpy()
    # the reference against itself in float64, same draws
    m64 = ref.VNet(in_channels=cin, num_classes=1)
    m64.load_state_dict(sd0)
    m64 = m64.double()
    ad64 = None if rec.adapter is None else (rec.adapter[0].double(), rec.adapter[1].double())
    l64, loss64, _, gn64 = step(m64, x.double(), mask.double(), Draws(m64, rec.masks, ad64))
    meta["ref_fp32_vs_fp64"] = {"logits_max_abs": (logits.double() - l64).abs().max().item(),
                                "logits_max_abs_over_max": ((logits.double() - l64).abs().max() / l64.abs().max()).item(),
                                "loss_abs": abs(loss - loss64), "global_grad_norm_rel": abs(gnorm - gn64) / gn64}
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **arrays)
    with open(os.path.join(OUT, f"{tag}.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(tag, "loss", loss, "gnorm", gnorm, meta["ref_fp32_vs_fp64"])


def main() -> None:
    ref = load_reference("vnet")["vnet"]
    torch.manual_seed(0)
    write_manifest(ref.VNet(), "vnet")
    run_case(ref, 1, "vnet_b2_64", True)
    run_case(ref, 3, "vnet_c3_b2_64", False)


if __name__ == "__main__":
    main()
