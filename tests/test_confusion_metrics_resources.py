"""CPU guard on the confusion-metric kernels as compiled (tools/kres.py, a gfx950 cross-compile): no vector register spills and
no scratch.  Nothing else is read from the assembly."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# the counting kernels come in two forms each: 16 bytes per lane and 4 bytes per lane
KERNELS = {"confusion_clear_kernel": 1, "confusion_binary_kernel": 2, "confusion_class_kernel": 2, "confusion_finalize_binary_kernel": 1,
           "confusion_finalize_class_kernel": 1}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_confusion.hip"], jobs=1)


def test_confusion_kernels_have_no_spill_and_no_scratch(kernels):
    names = [k["demangled"] for k in kernels]
    for want, count in KERNELS.items():
        assert sum(want in n for n in names) == count, (want, names)
    assert len(kernels) == sum(KERNELS.values())
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
