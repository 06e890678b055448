"""CPU guard on the compiled window-attention kernels (tools/kres.py, a gfx950 cross-compile): uz_winattn.hip holds exactly
the eight kernels below -- the ones attn_plan() can select, so an instantiation that no plan reaches fails here -- each uses
no scratch and spills no vector register, and `slots` workgroups of each -- the constant its grid is sized by (ATTN_SLOTS_* /
UZ_WIDE_SLOTS_*, read from uz_winattn.hip here) -- fit a CU: slots x LDS <= 160 KB, and slots x (waves per workgroup / 4
SIMDs) x registers <= 512 per SIMD lane."""
import os
import re
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

SOURCE = "uz_winattn.hip"
WAVES_PER_WORKGROUP = 4          # 256 threads
# kernel symbol (Itanium mangling: I<type>E = the template argument, DF16b = __bf16, f = float; the leading number is the
# length of the name, so "winattn_fwd_kernel" cannot match "winattn_wide_fwd_kernel") -> the slots constant of its grid
KERNELS = {
    "23winattn_wide_fwd_kernelIDF16bE": "UZ_WIDE_SLOTS_FWD",
    "23winattn_wide_fwd_kernelIfE": "UZ_WIDE_SLOTS_FWD",
    "23winattn_wide_bwd_kernelIDF16bE": "UZ_WIDE_SLOTS_BWD_BF16",
    "23winattn_wide_bwd_kernelIfE": "UZ_WIDE_SLOTS_BWD_F32",
    "18winattn_fwd_kernelIfE": "ATTN_SLOTS_FWD",
    "24winattn_fwd_mfma2_kernel": "ATTN_SLOTS_FWD_MFMA2",
    "18winattn_bwd_kernelIfE": "ATTN_SLOTS_BWD",
    "23winattn_bwd_mfma_kernel": "ATTN_SLOTS_BWD_MFMA",
}


def _slots():
    text = open(os.path.join(kres.CSRC, SOURCE)).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr int (\w+_SLOTS_\w+) = (\d+);", text)}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return [k for k in kres.collect([SOURCE], jobs=1) if "winattn" in k["name"]]


def test_window_attention_kernels_are_the_selectable_ones_and_fit(kernels):
    slots = _slots()
    assert set(KERNELS.values()) == set(slots), slots
    by_name = {}
    for k in kernels:
        for sub in KERNELS:
            if sub in k["name"]:
                by_name[sub] = k
    assert set(by_name) == set(KERNELS), set(KERNELS) - set(by_name)
    assert len(kernels) == len(KERNELS), sorted(k["name"] for k in kernels)
    for sub, k in by_name.items():
        s = slots[KERNELS[sub]]
        regs, lds = k["vgpr_count"], k.get("group_segment_fixed_size", 0)      # vgpr_count includes the accumulator registers
        print(f"  {sub}: {regs} registers, {lds} B LDS, {s} slots")
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, sub
        assert s * lds <= 160 * 1024, (sub, s, lds)
        assert s * (WAVES_PER_WORKGROUP // 4) * regs <= 512, (sub, s, regs)
