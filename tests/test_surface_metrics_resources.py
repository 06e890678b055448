"""CPU guard on the surface-metric kernels as compiled (tools/kres.py, a gfx950 cross-compile): no vector register spills and
no scratch.  Nothing else is read from the assembly."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

KERNELS = ("surface_clear_kernel", "surface_codes_kernel", "surface_rows_kernel", "surface_columns_kernel", "surface_select1_kernel",
           "surface_level2_kernel", "surface_finalize_kernel")


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_surface.hip"], jobs=1)


def test_surface_kernels_have_no_spill_and_no_scratch(kernels):
    names = [k["demangled"] for k in kernels]
    for want in KERNELS:
        assert sum(want in n for n in names) == (2 if want == "surface_codes_kernel" else 1), (want, names)   # codes: one per mode
    assert len(kernels) == len(KERNELS) + 1
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
