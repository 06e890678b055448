"""GPU: a lazy activation -- conv_bn_relu(defer_apply=...) left the apply pass to its one reader -- is refused by every engine
block but that reader, and by that reader the second time.  The refusals are Python assertions in front of the launch: no
kernel is given the un-normalised buffer.  Shape: the smallest batch at which a 64 -> 64 channel layer at 64 x 64 takes the
folded route (512-pixel tiles over at least half of the CUs: N = 16)."""
import pytest
import torch
import torch.nn as nn

from unet_zoo_amd import ops
from unet_zoo_amd.engine import Engine

pytestmark = pytest.mark.gpu


def test_lazy_activation_goes_to_its_reader_once_and_nowhere_else():
    torch.manual_seed(0)
    dev = torch.device("cuda")
    conv1, conv2 = (nn.Conv2d(64, 64, 3, padding=1).to(dev) for _ in range(2))
    bn1, bn2 = (nn.BatchNorm2d(64).to(dev) for _ in range(2))
    eng = Engine(torch.bfloat16, dev, True, True)
    x = ops.act_from_nchw(torch.randn(16, 64, 64, 64, device=dev), torch.bfloat16)
    act, pooled = eng.conv_bn_relu(x, conv1, bn1, defer_apply=conv2)
    assert act.lazy is not None and pooled is None, "the layer did not take the folded route: nothing below would be tested"
    tape = len(eng.tape)
    with pytest.raises(AssertionError):
        eng.max_pool2x2(act)
    with pytest.raises(AssertionError):
        eng.add(act, act)
    with pytest.raises(AssertionError):
        act.window(0, 32)
    assert len(eng.tape) == tape                     # a refused block leaves no tape entry behind
    out, _ = eng.conv_bn_relu(act, conv2, bn2, sole_reader=True)
    assert out.lazy is None and (out.N, out.H, out.W, out.C) == (16, 64, 64, 64)
    with pytest.raises(AssertionError):
        eng.conv_bn_relu(act, conv2, bn2, sole_reader=True)
    torch.cuda.synchronize()
    assert torch.isfinite(out.dense()).all()
