"""CPU: VNet through the registry (unet_zoo/models/vnet.py, models/__init__.py:150-154): construction, kwarg mapping,
parameter count, the seed-0 state_dict against the reference's manifest, the config path, the refusals in the model, and
the descriptor checks of the k = 5 convolution family in the C ABI (the library loads without a GPU)."""
import ctypes
import hashlib
import json
import os

import pytest
import torch
import yaml

import unet_zoo_amd
from unet_zoo_amd import _lib
from unet_zoo_amd.config import Config
from unet_zoo_amd.models import VNet, hip_models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
N_PARAMS = 9_360_339

# the reference's default_train_config.yaml, cut down to two models
CFG_YAML = """
general: {project_name: "UNetZooTraining", working_dir: "./training_runs"}
data: {dataset_dir: "/data/jupyter_folder/pano_unet_bone/bone_mask", num_workers: 4, image_size: 512}
training: {epochs: 80, batch_size: 4, learning_rate: 0.0001, early_stopping_patience: 20, lr_scheduler_patience: 8,
           lr_scheduler_factor: 0.2, min_lr: 1e-7, num_classes: 1}
gpu: {use_multi_gpu: false, gpu_ids: [0, 1, 2, 3, 4, 5, 6, 7], single_gpu_id: 0}
models:
  names: [unet, vnet]
  params: {unet: {depth: 5}, vnet: {elu: true, nll: false}}
"""


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _count(m):
    return sum(p.numel() for p in m.parameters())


def test_vnet_builds_through_the_registry():
    assert "vnet" in hip_models()
    m = unet_zoo_amd.create_model("vnet")
    assert type(m) is VNet and "VNet" in unet_zoo_amd.models.__all__
    assert m.in_tr.conv1.in_channels == 3 and m.out_tr.conv1.out_channels == 1      # the registry's defaults
    k = unet_zoo_amd.create_model("VNet", in_channels=1, num_classes=2, nll=True, elu=True)
    assert k.in_tr.conv1.in_channels == 1 and k.out_tr.conv1.out_channels == 2
    assert not hasattr(k, "nll")                                                   # accepted, stored nowhere
    with pytest.raises(TypeError):
        unet_zoo_amd.create_model("vnet", not_an_option=1)


def test_parameter_count_and_module_tree():
    m = VNet()
    assert _count(m) == N_PARAMS and len(m.state_dict()) == 168
    assert [len(t.ops) for t in (m.down_tr32, m.down_tr64, m.down_tr128, m.down_tr256)] == [1, 2, 3, 2]
    assert [len(t.ops) for t in (m.up_tr256, m.up_tr128, m.up_tr64, m.up_tr32)] == [2, 2, 1, 1]
    assert not any(n.startswith("_forced") for n, _ in m.named_parameters())


def test_seed0_state_dict_matches_the_reference_manifest():
    with open(os.path.join(GOLDEN, "vnet_manifest.json")) as f:
        man = json.load(f)
    torch.manual_seed(0)
    sd = VNet().state_dict()
    assert list(sd.keys()) == [e[0] for e in man["entries"]]
    for k, shape, dtype, digest in man["entries"]:
        v = sd[k]
        assert list(v.shape) == shape and str(v.dtype) == "torch." + dtype
        assert _sha(v) == digest, f"seed-0 init of {k} differs from the reference"
    assert man["n_params"] == N_PARAMS


def test_prelu_is_refused_at_construction():
    with pytest.raises(NotImplementedError, match="elu=False"):
        unet_zoo_amd.create_model("vnet", elu=False)


def test_config_model_kwargs_build_vnet(tmp_path):
    d = yaml.safe_load(CFG_YAML)
    d["general"]["working_dir"] = str(tmp_path)
    c = Config(d)
    assert c.MODELS_TO_TRAIN == ["unet", "vnet"]
    m = unet_zoo_amd.create_model("vnet", **c.model_kwargs("vnet"))
    # the registry's default in_channels = 3: the 5x5 input layer has two more input planes than the 1-channel default
    assert type(m) is VNet and m.in_tr.conv1.in_channels == 3 and _count(m) == N_PARAMS + 2 * 16 * 25


def test_bad_inputs_are_refused_before_any_kernel():
    m = VNet(in_channels=1)
    with pytest.raises(ValueError, match="multiples of 16"):
        m.emit(None, torch.zeros(2, 1, 40, 40))
    with pytest.raises(ValueError, match="more than 1 value per channel"):
        m.emit(None, torch.zeros(1, 1, 16, 16))
    with pytest.raises(ValueError, match="expected a"):
        m.emit(None, torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError, match="8 masks"):
        m.force_draws(dropout=[torch.ones(2, 128)])


def test_cpu_forward_raises_like_every_other_model():
    m = VNet(in_channels=1)
    with pytest.raises(_lib.HipLibraryError):
        m(torch.zeros(2, 1, 32, 32))


def _c5(dtype=_lib.UZ_BF16, N=2, H=16, W=16, Cin=32, ldx=None, Nout=32, ldy=None, ksize=5):
    return _lib.Conv5Desc(dtype, N, H, W, Cin, Cin if ldx is None else ldx, Nout, Nout if ldy is None else ldy, ksize)


@pytest.mark.parametrize("kw,word", [(dict(Cin=12), b"Cin"), (dict(Cin=36, dtype=_lib.UZ_BF16), b"Cin"), (dict(Cin=1024), b"Cin"),
                                     (dict(Nout=1024), b"Nout"), (dict(ksize=3), b"kernel size"), (dict(ksize=7), b"kernel size"),
                                     (dict(ldx=20), b"ldx"), (dict(ldy=16), b"ldy"), (dict(dtype=5), b"dtype")])
def test_conv5x5_descriptor_check_refuses_without_a_gpu(kw, word):
    lib = _lib.load()
    assert lib.uz_conv5x5_grid_m(ctypes.byref(_c5(**kw))) == -1
    assert word in lib.uz_last_error_string()
    # the launch entry point makes the same check before it touches a pointer
    assert lib.uz_conv5x5(ctypes.byref(_c5(**kw)), None, None, None, None, None, None) == -1


@pytest.mark.parametrize("C", [32, 64, 128, 256])
@pytest.mark.parametrize("dtype", [_lib.UZ_F32, _lib.UZ_BF16])
def test_vnet_layer_shapes_pass_the_descriptor_checks(C, dtype):
    lib = _lib.load()
    assert lib.uz_conv5x5_grid_m(ctypes.byref(_c5(dtype=dtype, Cin=C, Nout=C))) > 0
    w = _lib.Wgrad5Desc(dtype, 2, 16, 16, C, C, C, C, 5, C, C)
    assert lib.uz_wgrad5x5_workspace_bytes(ctypes.byref(w)) > 0
    assert lib.uz_conv5x5_grid_m(ctypes.byref(_c5(dtype=dtype, Cin=32, Nout=1, ldy=8))) > 0     # the output layer


@pytest.mark.parametrize("fields,word", [((2, 16, 16, 12, 12, 32, 32, 5, 12, 32), b"multiples"),
                                         ((2, 16, 16, 32, 32, 32, 32, 3, 32, 32), b"kernel size"),
                                         ((2, 16, 16, 32, 32, 32, 32, 5, 40, 32), b"result channels"),
                                         ((2, 16, 16, 640, 640, 32, 32, 5, 32, 32), b"at most 512")])
def test_wgrad5x5_descriptor_check_refuses_without_a_gpu(fields, word):
    lib = _lib.load()
    d = _lib.Wgrad5Desc(_lib.UZ_BF16, *fields)
    assert lib.uz_wgrad5x5_workspace_bytes(ctypes.byref(d)) == -1
    assert word in lib.uz_last_error_string()
    assert lib.uz_wgrad5x5(ctypes.byref(d), None, None, None, None, None) == -1


def test_bn_elu_refuses_bad_arguments_without_a_gpu():
    lib = _lib.load()
    assert lib.uz_bn_elu_apply(_lib.UZ_BF16, None, 32, None, None, 2, 64, 32, None, 0, None, 32, None, 0, None, 0, None) == -1
    assert b"null" in lib.uz_last_error_string()
    assert lib.uz_bn_elu_apply(_lib.UZ_BF16, None, 32, None, None, 2, 64, 32, None, 0, None, 32, None, 0, None, 4, None) == -1
    assert b"flags" in lib.uz_last_error_string()
    d = _lib.BnEluBwdDesc(_lib.UZ_BF16, 2, 64, 32, 16, 32, 32, 0, 0, 32, 0, 3)
    assert lib.uz_bn_elu_bwd_rows(ctypes.byref(d)) == -1
    assert b"leading dimension" in lib.uz_last_error_string()
    # a second gradient narrower than the tensor, and a misaligned tensor on the 16-byte vector path (0x1000 is never read:
    # the checks come before any launch)
    p = 0x1000
    d = _lib.BnEluBwdDesc(_lib.UZ_BF16, 2, 64, 32, 32, 32, 32, 16, 0, 32, 0, 1)
    assert lib.uz_bn_elu_bwd_reduce(ctypes.byref(d), p, None, p, p, None, None, p, p, p, p, p, None) == -1
    assert b"g1" in lib.uz_last_error_string()
    d = _lib.BnEluBwdDesc(_lib.UZ_BF16, 2, 64, 32, 32, 32, 32, 0, 0, 32, 0, 1)
    assert lib.uz_bn_elu_bwd_reduce(ctypes.byref(d), p + 8, None, p, None, None, None, p, p, p, p, p, None) == -1
    assert b"aligned" in lib.uz_last_error_string()
    assert lib.uz_bn_elu_apply(_lib.UZ_BF16, p + 8, 32, p, p, 2, 64, 32, None, 0, p, 32, None, 0, None, 1, None) == -1
    assert b"aligned" in lib.uz_last_error_string()
