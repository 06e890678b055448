"""CPU guard on the boundary-loss kernels as compiled (tools/kres.py, a gfx950 cross-compile): no vector register spills and
no scratch.  Nothing else is read from the assembly."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# kernel -> instances (rows and loss: one per mode)
KERNELS = {"boundary_planes_kernel": 1, "boundary_rows_kernel": 2, "boundary_columns_kernel": 1, "boundary_loss_kernel": 2,
           "boundary_finalize_kernel": 1}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_boundary_loss.hip"], jobs=1)


def test_boundary_kernels_have_no_spill_and_no_scratch(kernels):
    names = [k["demangled"] for k in kernels]
    for want, count in KERNELS.items():
        assert sum(want in n for n in names) == count, (want, names)
    assert len(kernels) == sum(KERNELS.values())
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
        assert k.get("group_segment_fixed_size", 0) <= 160 * 1024, k["demangled"]
