"""CPU guard on the patch kernels as compiled (tools/kres.py, a gfx950 cross-compile): no vector register spills, no scratch,
no LDS, and the cut kernel keeps the loads of a run in flight together -- every load is unconditional from a clamped address
and the zero of a patch without a picture is selected afterwards (a load written under a branch is closed by
s_waitcnt vmcnt(0) where the branch ends)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# most load -> vmcnt(0) -> load points in a cut kernel.  The picture's C x 4 loads and the first mask plane's 4 are issued
# together and waited for once; the further planes of a multi-channel fp32 mask are loaded in a loop behind them, one wait per
# plane inside ONE loop body: that is the single point (the forms without a mask or with labels show none).  The coordinates
# and the normalisation are scalar loads.
LOAD_WAIT_BOUND = 1


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_patch.hip"], jobs=1)


def test_patch_kernels_have_no_spill_and_no_scratch(kernels):
    names = [k["demangled"] for k in kernels]
    assert sum("patch_cut_kernel" in n for n in names) == 24          # C = 1..4 x (fp32, uint8) x (no mask, fp32 mask, int32 labels)
    for one in ("patch_count_kernel", "patch_scan_kernel", "patch_draw_kernel"):
        assert sum(one in n for n in names) == 1, one
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
        assert k.get("group_segment_fixed_size", 0) == 0, k["demangled"]  # no LDS
        assert k["vgpr_count"] <= 256, (k["demangled"], k["vgpr_count"])


def test_cut_kernel_keeps_its_loads_in_flight(kernels):
    bad = []
    for k in kernels:
        if "patch_cut_kernel" in k["demangled"]:
            # four pixels of a run at the least: the loads are there, and not behind one wait each
            assert k["loads"] >= 4, (k["demangled"], k["loads"])
            if k["load_wait_points"] > LOAD_WAIT_BOUND:
                bad.append(f"{kres.short(k['demangled'])}: {k['load_wait_points']} load -> vmcnt(0) -> load points "
                           f"(bound {LOAD_WAIT_BOUND}, {k['loads']} loads)")
    assert not bad, "kernels whose loads are waited for one by one (DESIGN 3h):\n" + "\n".join(bad)
