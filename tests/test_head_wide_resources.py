"""CPU guard on the wide head's kernels as compiled (tools/kres.py, a gfx950 cross-compile): no vector register spills, no
scratch, at most 256 vector registers, LDS within what two workgroups per CU allow (the persistent grid is two workgroups
per CU), and a forward whose loads are in flight together."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

LDS_PER_CU = 160 * 1024
# most load -> vmcnt(0) -> load points in a forward kernel.  The weights (register forms), the bias and the four pixels'
# activation vectors of a trip are written as unconditional loads from clamped addresses and issued together: no point.
# The forms with the weights in LDS walk the channel vectors in a loop whose body fetches the NEXT vector before it
# multiplies the present one; the wait at the top of that body stands between the prologue's loads and the loop's: one point.
FWD_LOAD_WAIT_BOUND = 1


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_head_wide.hip"], jobs=1)


def test_every_form_is_there(kernels):
    names = [k["demangled"] + " " + k["name"] for k in kernels]
    assert sum("head_wide_fwd_kernel" in n for n in names) == 12      # (bf16, fp32) x (16, 32 classes) x (1, 2 vectors in registers, LDS)
    assert sum("head_wide_bwd_kernel" in n for n in names) == 4       # (bf16, fp32) x (16, 32 classes)
    assert sum("head_wide_finalize_kernel" in n for n in names) == 1


def test_no_spill_no_scratch_and_lds_for_two_workgroups_per_cu(kernels):
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
        assert k["vgpr_count"] <= 256, (k["demangled"], k["vgpr_count"])
        assert 2 * k.get("group_segment_fixed_size", 0) <= LDS_PER_CU, (k["demangled"], k.get("group_segment_fixed_size"))


def test_forward_keeps_its_loads_in_flight(kernels):
    bad = []
    for k in kernels:
        if "head_wide_fwd_kernel" in k["demangled"] + k["name"]:
            assert k["loads"] >= 4, (k["demangled"], k["loads"])      # four pixels of a wave's run at the least
            if k["load_wait_points"] > FWD_LOAD_WAIT_BOUND:
                bad.append(f"{kres.short(k['demangled'])}: {k['load_wait_points']} load -> vmcnt(0) -> load points "
                           f"(bound {FWD_LOAD_WAIT_BOUND}, {k['loads']} loads)")
    assert not bad, "kernels whose loads are waited for one by one (DESIGN 3h):\n" + "\n".join(bad)
