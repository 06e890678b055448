"""CPU guard on the k = 5 family's compiled kernels (tools/kres.py, a gfx950 cross-compile): the loads of a K-step / of an
element stay in flight together (a load written under a branch is closed by s_waitcnt vmcnt(0) where the branch
ends), no vector register spills, no scratch, and the LDS of two workgroups fits a CU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# (substring of the mangled / demangled name) -> most load -> vmcnt(0) -> load points: the prologue step and the step inside
# the K loop for the two MFMA kernels; the parameter prologue and the element loads for the element passes
LOAD_WAIT_BOUNDS = {
    "conv5_kernel": 2,
    "wgrad5_kernel": 2,
    "bn_elu_apply_kernel": 2,
    "bn_elu_bwd_reduce_kernel": 2,
    "bn_elu_bwd_apply_kernel": 2,
}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_conv5x5.hip"], jobs=1)


def test_k5_kernels_keep_their_loads_in_flight(kernels):
    bad, seen = [], set()
    for k in kernels:
        for sub, bound in LOAD_WAIT_BOUNDS.items():
            if sub in k["name"] or sub in k["demangled"]:
                seen.add(sub)
                if k["load_wait_points"] > bound:
                    bad.append(f"{kres.short(k['demangled'])}: {k['load_wait_points']} load -> vmcnt(0) -> load points "
                               f"(bound {bound}, {k['loads']} loads)")
    assert seen == set(LOAD_WAIT_BOUNDS), set(LOAD_WAIT_BOUNDS) - seen
    assert not bad, "kernels whose loads are waited for one by one (DESIGN 3h):\n" + "\n".join(bad)


def test_k5_kernels_resources(kernels):
    mfma = [k for k in kernels if "conv5_kernel" in k["name"] + k["demangled"] or "wgrad5_kernel" in k["name"] + k["demangled"]]
    assert len(mfma) == 10          # 3 forward tiles + 2 weight-gradient tiles, bf16 and fp32
    for k in kernels:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
    for k in mfma:                  # __launch_bounds__(256, 2): two workgroups per CU
        assert k["vgpr_count"] <= 256, (k["demangled"], k["vgpr_count"])
        assert 2 * k.get("group_segment_fixed_size", 0) <= 160 * 1024, k["demangled"]
