"""Generate the UNeXt goldens under tests/golden/ from the reference's own unext.py (build machine only: the reference
tree is not on the GPU machines).  Uses oracle.gen_golden's loader, case runner and manifest writer unchanged.

    python tools/gen_golden_unext.py

Writes unext_manifest.json / unext_s_manifest.json (seed-0 SHA-256 per state_dict tensor), unext_b2_64 and
unext_s_b2_64 (train + eval logits, loss, gradient norms, sampled gradients), unext_s_b1_100 (an odd size: 25 x 25,
13 x 13 and 7 x 7 token maps, which the reduction convolutions r = 8 / 4 / 2 crop) and unext_s_b1_96x160 (a non-square
input: 24 x 40 tokens after the stride-4 embedding); the last two with sampled logits only."""
import os
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from oracle.gen_golden import load_reference, run_case, write_manifest  # noqa: E402


def main() -> None:
    ref = load_reference("unext")["unext"]
    for name, cls in (("unext", ref.UNext), ("unext_s", ref.UNext_S)):
        torch.manual_seed(0)
        model = cls(input_channels=3, num_classes=1, img_size=64)
        write_manifest(model, name)
        run_case(model, 2, 64, 64, f"{name}_b2_64", full_logits=True, name=name, bn_keys=())
    torch.manual_seed(0)
    model = ref.UNext_S(input_channels=3, num_classes=1, img_size=100)
    run_case(model, 1, 100, 100, "unext_s_b1_100", full_logits=False, name="unext_s", bn_keys=())
    torch.manual_seed(0)
    model = ref.UNext_S(input_channels=3, num_classes=1, img_size=96)
    run_case(model, 1, 96, 160, "unext_s_b1_96x160", full_logits=False, name="unext_s", bn_keys=())


if __name__ == "__main__":
    main()
