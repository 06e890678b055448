"""CPU guard on the step-tail kernels as compiled (tools/kres.py, a gfx950 cross-compile): the expected instances, no vector
register spills and no scratch.  Nothing else is read from the assembly."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# kernel -> instances: the norm with / without the accumulator, the prepare launch per schedule form, the apply pass for
# (acc, ema) in all four combinations, the accumulate pass that overwrites / adds
KERNELS = {"tail_sqnorm_kernel": 2, "tail_prepare_kernel": 4, "tail_apply_kernel": 4, "tail_accumulate_kernel": 2,
           "tail_swap_kernel": 1}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_steptail.hip"], jobs=1)


def test_steptail_kernels_have_no_spill_and_no_scratch(kernels):
    names = [k["demangled"] for k in kernels]
    for want, count in KERNELS.items():
        assert sum(want in n for n in names) == count, (want, names)
    assert len(kernels) == sum(KERNELS.values())
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
