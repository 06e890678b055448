"""CPU guard on the augmentation kernels as compiled (tools/kres.py, a gfx950 cross-compile): no vector register spills, no
scratch, and the taps of an element stay in flight together -- every load is unconditional from a clamped address and the
fill is selected afterwards (a load written under a branch is closed by s_waitcnt vmcnt(0) where the branch ends)."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# most load -> vmcnt(0) -> load points: the displacement grid's taps in front of the picture's (the sample's parameters are
# scalar loads), and the picture's in front of the further planes of a multi-channel mask
LOAD_WAIT_BOUND = 2


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_augment.hip"], jobs=1)


def test_augment_kernels_have_no_spill_and_no_scratch(kernels):
    names = [k["demangled"] for k in kernels]
    assert sum("augment_apply_kernel" in n for n in names) == 12          # C = 1..4 x (no mask, fp32 mask, int32 labels)
    assert sum("augment_params_kernel" in n for n in names) == 1
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
        assert k.get("group_segment_fixed_size", 0) == 0, k["demangled"]  # no LDS
        assert k["vgpr_count"] <= 256, (k["demangled"], k["vgpr_count"])


def test_apply_kernel_keeps_its_taps_in_flight(kernels):
    bad = []
    for k in kernels:
        if "augment_apply_kernel" in k["demangled"]:
            # C x 4 pixels x 4 taps at the least: the taps are there, and not behind one wait each
            assert k["loads"] >= 16, (k["demangled"], k["loads"])
            if k["load_wait_points"] > LOAD_WAIT_BOUND:
                bad.append(f"{kres.short(k['demangled'])}: {k['load_wait_points']} load -> vmcnt(0) -> load points "
                           f"(bound {LOAD_WAIT_BOUND}, {k['loads']} loads)")
    assert not bad, "kernels whose loads are waited for one by one (DESIGN 3h):\n" + "\n".join(bad)
