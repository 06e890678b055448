"""CPU: the surface of the graphed evaluation pass and of the convolutions with the eval-mode BatchNorm in their epilogue --
the header declares the new entries and the library exports them, GraphedEval refuses what it cannot run before any GPU
call, the _supported queries answer without a GPU, and the new kernel instantiations keep the resources of their plain
siblings (tools/kres.py: a gfx950 cross-compile read from the code-object metadata)."""
import ctypes
import os
import re
import sys
from ctypes import byref

import pytest
import torch

import unet_zoo_amd
from unet_zoo_amd import _lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import kres  # noqa: E402

NEW = ("uz_conv_igemm_bnact_supported", "uz_conv_igemm_bnact", "uz_conv3x3_first_fwd_bnact")


def test_header_declares_and_library_exports_the_new_entries():
    with open(os.path.join(ROOT, "include", "unetzoo_hip.h")) as f:
        header = f.read()
    lib = ctypes.CDLL(L.LIB_PATH)
    for name in NEW:
        assert re.search(r"\bint\s+" + name + r"\s*\(", header), name
        assert name in L.EXPORTS
        assert getattr(lib, name) is not None


def test_graphed_eval_is_exported():
    assert unet_zoo_amd.GraphedEval is not None and "GraphedEval" in unet_zoo_amd.__all__
    from unet_zoo_amd.engine import Engine
    assert Engine.fold_bn_eval is False


def test_train_mode_and_cpu_models_raise_before_any_gpu_call():
    m = unet_zoo_amd.create_model("unet", in_channels=3, num_classes=1)
    x, t = torch.zeros(1, 3, 16, 16), torch.zeros(1, 1, 16, 16)
    ev = unet_zoo_amd.GraphedEval(m.train(), "bce_dice", fold_bn=True)
    with pytest.raises(RuntimeError, match="model.eval"):
        ev(x, t)
    ev = unet_zoo_amd.GraphedEval(m.eval(), "bce_dice", fold_bn=True)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev(x, t)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.evaluate([(x, t)])
    with pytest.raises(ValueError):
        unet_zoo_amd.GraphedEval(m, "dice")
    with pytest.raises(TypeError):
        unet_zoo_amd.GraphedEval(torch.nn.Conv2d(3, 3, 3))


def _desc(dt, N, H, W, Cin, Cout, ldy, up=False, ntaps=9):
    return L.ConvDesc(L.dtype_code(dt), N, H, W, H // 2 if up else H, W // 2 if up else W, Cin, Cin, Cout, ldy, ntaps,
                      L.TAPS_CONV_UP2 if up else L.TAPS_CONV, 1, L.STORE_PLAIN, 0, 0, 0)


def test_supported_queries_answer_on_the_cpu():
    lib = L.load()
    B, F = torch.bfloat16, torch.float32
    yes = [_desc(B, 2, 32, 32, 64, 64, 64), _desc(B, 1, 24, 40, 64, 128, 128), _desc(B, 1, 16, 16, 128, 64, 128),
           _desc(B, 1, 16, 16, 64, 64, 64, up=True), _desc(F, 1, 16, 16, 32, 32, 32), _desc(F, 1, 12, 20, 32, 64, 64),
           _desc(B, 16, 256, 256, 64, 64, 64), _desc(B, 16, 128, 128, 64, 128, 128)]          # unet's level-1 / level-2 maps
    for d in yes:
        assert lib.uz_conv_igemm_bnact_supported(byref(d)) == 1, [getattr(d, n) for n, _ in d._fields_]
    code = L.dtype_code(B)
    no = [L.ConvDesc(code, 1, 8, 8, 8, 8, 64, 64, 128, 32, 1, L.TAPS_CONV, 1, L.STORE_SHUFFLE2X2, 32, 0, 0),     # shuffle store
          L.ConvDesc(code, 1, 8, 8, 16, 16, 64, 64, 128, 128, 4, L.TAPS_GATHER2X2, 1, L.STORE_PLAIN, 0, 0, 0),   # gather
          _desc(B, 1, 8, 8, 64, 128, 128, ntaps=1),                                                            # 1x1 on gemm_dma
          _desc(B, 16, 16, 16, 1024, 512, 512),                                                                # split-K plan
          _desc(B, 2, 64, 64, 32, 64, 64)]                                                    # weights-in-registers kernel
    for d in no:
        assert lib.uz_conv_igemm_bnact_supported(byref(d)) == 0, [getattr(d, n) for n, _ in d._fields_]
    assert lib.uz_conv_igemm_bnact_supported(None) == 0


@pytest.fixture(scope="module")
def kernels():
    if not os.path.exists(kres.HIPCC):
        pytest.skip("no hipcc")
    return kres.collect(["uz_igemm.hip", "uz_conv3x3.hip", "uz_conv3x3_pp.hip", "uz_conv_first.hip"], jobs=4)


def _occupancy(k):
    """(waves per SIMD the registers allow, workgroups per CU the LDS allows): 512 registers per SIMD lane in blocks of 8,
    160 KB of LDS per CU"""
    v = (k["vgpr_count"] + 7) // 8 * 8
    lds = k.get("group_segment_fixed_size", 0)
    return min(8, 512 // v), (160 * 1024 // lds if lds else 99)


# the output activation is the LAST template flag of each of the four kernel templates: an instantiation whose mangled name
# ends its template arguments with `Lb1E` is an ACT form, and the same name with `Lb0E` there is its plain sibling
FAMILIES = {"igemm_kernel": 4,             # two tiles x two dtypes
            "conv3x3_direct_kernel": 12,   # six tile / residency forms x two dtypes
            "conv3x3_pp_kernel": 5,        # the five ping-pong tile configurations
            "conv_first_fwd_kernel": 2}    # 32 and 64 output channels


def test_act_instantiations_keep_the_resources_of_their_plain_siblings(kernels):
    by = {k["name"]: k for k in kernels}
    seen = {f: 0 for f in FAMILIES}
    for n, a in by.items():
        m = re.match(r"^(.*)Lb1E(EEv.*)$", n)
        fam = [f for f in FAMILIES if f + "I" in n]
        if not m or not fam:
            continue
        plain = m.group(1) + "Lb0E" + m.group(2)
        assert plain in by, (n, plain)
        p = by[plain]
        assert a.get("vgpr_spill_count", 0) == 0 and a.get("private_segment_fixed_size", 0) == 0, n
        # the occupancy the resources allow is the sibling's (a form that drops the statistics may need LESS: never more)
        oa, op = _occupancy(a), _occupancy(p)
        assert oa[0] >= op[0] and oa[1] >= op[1], (n, oa, op)
        seen[fam[0]] += 1
    assert seen == FAMILIES
