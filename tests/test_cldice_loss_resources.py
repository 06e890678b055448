"""CPU guard on the clDice kernels as compiled (tools/kres.py, a gfx950 cross-compile): the expected kernel instances, no
vector register spills, no scratch, LDS within 160 KB (the backward instance for 10 iterations holds five fp32 images and
one 16-bit image of an 80 x 80 region).  Nothing else is read from the assembly."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# kernel -> instances (forward: three sizes of the LDS region x (map, target); backward: the three sizes; prob and grad: one
# kernel per mode)
KERNELS = {"cldice_forward_kernel": 6, "cldice_backward_kernel": 3, "cldice_prob_binary_kernel": 1, "cldice_prob_class_kernel": 1,
           "cldice_sums_kernel": 1, "cldice_grad_binary_kernel": 1, "cldice_grad_class_kernel": 1}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_cldice_loss.hip"], jobs=1)


def test_cldice_kernels_have_no_spill_and_no_scratch(kernels):
    names = [k["demangled"] for k in kernels]
    for want, count in KERNELS.items():
        assert sum(want in n for n in names) == count, (want, names)
    assert len(kernels) == sum(KERNELS.values())
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
        assert k.get("group_segment_fixed_size", 0) <= 160 * 1024, k["demangled"]
    # the images are static LDS: the largest backward instance is what bounds the tile
    assert max(k.get("group_segment_fixed_size", 0) for k in kernels) > 128 * 1024
