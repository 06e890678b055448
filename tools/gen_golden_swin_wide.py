"""Generate the wide-window Swin-UNet V2 goldens under tests/golden/ from the reference's own swin_unet_v2.py (build machine
only: the reference tree is not on the GPU machines).  Uses oracle.gen_golden's loader, timm stand-in, manifest writer, hash
and index sampler unchanged.

    python tools/gen_golden_swin_wide.py

Writes swin_unet_v2_128_ws16_manifest.json (seed 0) and two fixtures, each a full train step (drop_path_rate 0) and the eval
logits of B = 2 images, with the fields of swin_unet_v2_b2_64_ws4:
    swin_unet_v2_b2_128_ws16   256-token windows on the 32^2 and 16^2 token maps (shift 0 and 8 on 32^2), 8 on 8^2, 4 on 4^2
    swin_unet_v2_b2_96_ws12    144-token windows on 24^2 (shift 0 and 6) and 12^2, then 6 and 3
Each json also holds `ref_fp32_vs_fp64`, the reference's own deviation between a float32 and a float64 run, and
`mask_excluded`: the pixels with |logit| <= 1e-3 max|logit|, whose sign a run within the 1e-3 logit bound may flip."""
import contextlib
import io
import json
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle.gen_golden import OUT, _timm_stand_in, load_reference, sample_idx, sha, write_manifest  # noqa: E402
from oracle.torch_ref import synthetic_batch  # noqa: E402

CASES = [(128, 16), (96, 12)]


def build(Ref, img, ws):
    torch.manual_seed(0)
    with contextlib.redirect_stdout(io.StringIO()):
        return Ref(img_size=img, in_chans=3, num_classes=1, window_size=ws, drop_path_rate=0.0)


def step(model, x, mask):
    model.train()
    model.zero_grad()
    logits = model(x)
    loss = F.binary_cross_entropy_with_logits(logits, mask.to(logits.dtype))
    loss.backward()
    named = [(n, p) for n, p in model.named_parameters() if p.grad is not None]
    gnorm = torch.sqrt(sum((p.grad.double() ** 2).sum() for _, p in named)).item()
    return logits.detach(), loss.item(), named, gnorm


def run_case(Ref, img, ws):
    B, tag = 2, f"swin_unet_v2_b2_{img}_ws{ws}"
    model = build(Ref, img, ws)
    if (img, ws) == CASES[0]:
        write_manifest(model, f"swin_unet_v2_{img}_ws{ws}")
    sd0 = {k: v.clone() for k, v in model.state_dict().items()}
    x, mask = synthetic_batch(B, 3, img, img, seed=1)
    logits, loss, named, gnorm = step(model, x, mask)
    unused = [n for n, p in model.named_parameters() if p.grad is None]
    arrays = {"train_logits": logits.numpy()}
    meta = {"model": "swin_unet_v2", "B": B, "H": img, "W": img, "window_size": ws, "input_sha256": sha(x),
            "mask_sha256": sha(mask), "loss": loss, "global_grad_norm": gnorm,
            "grad_l2": {n: p.grad.double().norm().item() for n, p in named}, "unused_parameters": unused,
            "train_positive_pixels": int((logits > 0).sum().item()),
            "tau_shapes": [list(p.shape) for n, p in model.named_parameters() if n.endswith(".tau") and ".blocks.0." in n
                           and n.startswith("layers.")]}
    for n, p in named:
        gi = sample_idx(p.numel(), 64)
        arrays["gidx/" + n] = gi
        arrays["gval/" + n] = p.grad.flatten()[gi].numpy()
    model.eval()
    with torch.no_grad():
        ev = model(x)
    arrays["eval_logits"] = ev.numpy()
    meta["eval_positive_pixels"] = int((ev > 0).sum().item())
    meta["mask_excluded"] = {"train": int((logits.abs() <= 1e-3 * logits.abs().max()).sum().item()),
                             "eval": int((ev.abs() <= 1e-3 * ev.abs().max()).sum().item()), "of": logits.numel()}
    # the reference against itself in float64
    m64 = build(Ref, img, ws)
    m64.load_state_dict(sd0)
    m64 = m64.double()
    l64, loss64, _, gn64 = step(m64, x.double(), mask.double())
    meta["ref_fp32_vs_fp64"] = {"logits_max_abs_over_max": ((logits.double() - l64).abs().max() / l64.abs().max()).item(),
                                "loss_abs": abs(loss - loss64), "global_grad_norm_rel": abs(gnorm - gn64) / gn64}
    np.savez_compressed(os.path.join(OUT, f"{tag}.npz"), **arrays)
    with open(os.path.join(OUT, f"{tag}.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
    print(tag, "loss", loss, "gnorm", gnorm, "unused", len(unused), meta["tau_shapes"], meta["mask_excluded"],
          meta["ref_fp32_vs_fp64"])


def main() -> None:
    _timm_stand_in()
    Ref = load_reference("swin_unet_v2")["swin_unet_v2"].SwinTransformerSys
    for img, ws in CASES:
        run_case(Ref, img, ws)


if __name__ == "__main__":
    main()
