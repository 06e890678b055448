"""CPU guard on the post-processing and TTA kernels as compiled (tools/kres.py, a gfx950 cross-compile): every kernel is there
once per mode, no vector register spills and no scratch.  Nothing else is read from the assembly."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

# kernel -> instances: codes one per mode, init one per source of the set, compress with and without the counters
POSTPROC = {"postproc_clear_kernel": 1, "postproc_codes_kernel": 2, "postproc_init_kernel": 3, "postproc_merge_kernel": 1,
            "postproc_compress_kernel": 2, "postproc_fill_kernel": 1, "postproc_top_kernel": 1, "postproc_keep_kernel": 1,
            "postproc_scan_kernel": 1, "postproc_number_kernel": 1, "postproc_apply_kernel": 1, "postproc_finalize_kernel": 1,
            "postproc_classmap_kernel": 1}
# merge: (fp32, bf16) x (binary, class); decide: one per mode
TTA = {"tta_flip_kernel": 1, "tta_merge_kernel": 4, "tta_decide_kernel": 2}


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return {src: kres.collect([src], jobs=1) for src in ("uz_postproc.hip", "uz_tta.hip")}


@pytest.mark.parametrize("src,want", [("uz_postproc.hip", POSTPROC), ("uz_tta.hip", TTA)])
def test_kernels_are_all_there_without_spill_or_scratch(kernels, src, want):
    ks = kernels[src]
    names = [k["demangled"] for k in ks]
    for name, count in want.items():
        assert sum(name in n for n in names) == count, (name, names)
    assert len(ks) == sum(want.values())
    for k in ks:
        assert k.get("vgpr_spill_count", 0) == 0 and k.get("private_segment_fixed_size", 0) == 0, k["demangled"]
