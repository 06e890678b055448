"""CPU guard on the sliding-window kernels as compiled (tools/kres.py, a gfx950 cross-compile): every kernel instance is there, no
vector register spills and no scratch.  Nothing else is read from the assembly."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# blend: one instance per (slots along H, slots along W), each of 1, 2, 4, 8
TILE = {"tile_gather_kernel": 1, "tile_blend_kernel": 16}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_tile.hip"], jobs=1)


def test_kernels_are_all_there_without_spill_or_scratch(kernels):
    names = [k["demangled"] for k in kernels]
    for name, count in TILE.items():
        assert sum(name in n for n in names) == count, (name, names)
    for ky in (1, 2, 4, 8):
        for kx in (1, 2, 4, 8):
            assert sum(f"tile_blend_kernel<{ky}, {kx}>" in n for n in names) == 1, (ky, kx)
    assert len(kernels) == sum(TILE.values())
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
