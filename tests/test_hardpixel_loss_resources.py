"""CPU guard on the hard-pixel kernels as compiled (tools/kres.py, a gfx950 cross-compile): the expected kernel instances, no
vector register spills, no scratch (the class-mode kernels walk their K planes, K = 32 included: nothing per class is held),
LDS within 160 KB.  Nothing else is read from the assembly."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# kernel -> instances (loss and grad: one kernel per mode; hist and pick serve every round)
KERNELS = {"hardpixel_loss_binary_kernel": 1, "hardpixel_loss_class_kernel": 1, "hardpixel_hist_kernel": 1, "hardpixel_pick_kernel": 1,
           "hardpixel_grad_binary_kernel": 1, "hardpixel_grad_class_kernel": 1, "hardpixel_finalize_kernel": 1}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_hardpixel_loss.hip"], jobs=1)


def test_hardpixel_kernels_have_no_spill_and_no_scratch(kernels):
    names = [k["demangled"] for k in kernels]
    for want, count in KERNELS.items():
        assert sum(want in n for n in names) == count, (want, names)
    assert len(kernels) == sum(KERNELS.values())
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
        assert k.get("group_segment_fixed_size", 0) <= 160 * 1024, k["demangled"]
