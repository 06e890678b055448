"""CPU: UNeXt / UNeXt-S through the registry (unet_zoo/models/unext.py, models/__init__.py:185-199): construction,
kwarg mapping, parameter counts, the seed-0 state_dict against the reference's manifests, the config path, and the
refusals -- head sizes the attention kernels do not take, in the model and in the C ABI's descriptor check."""
import ctypes
import hashlib
import json
import os

import pytest
import torch
import torch.nn as nn
import yaml

import unet_zoo_amd
from unet_zoo_amd import _lib
from unet_zoo_amd.config import Config
from unet_zoo_amd.models import UNext, UNext_S, hip_models

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")

# the reference's default_train_config.yaml with the two UNeXt entries (models.names, params: unext: {} / unext_s: {})
CFG_YAML = """
general: {project_name: "UNetZooTraining", working_dir: "./training_runs"}
data: {dataset_dir: "/data/jupyter_folder/pano_unet_bone/bone_mask", num_workers: 4, image_size: 512}
training: {epochs: 80, batch_size: 4, learning_rate: 0.0001, early_stopping_patience: 20, lr_scheduler_patience: 8,
           lr_scheduler_factor: 0.2, min_lr: 1e-7, num_classes: 1}
gpu: {use_multi_gpu: false, gpu_ids: [0, 1, 2, 3, 4, 5, 6, 7], single_gpu_id: 0}
models:
  names: [unet, unext, unext_s]
  params: {unet: {depth: 5}, unext: {}, unext_s: {}}
"""


def _sha(t):
    return hashlib.sha256(t.detach().contiguous().cpu().numpy().tobytes()).hexdigest()


def _count(m):
    return sum(p.numel() for p in m.parameters())


def test_both_names_build_through_the_registry():
    assert {"unext", "unext_s"} <= set(hip_models())
    m = unet_zoo_amd.create_model("unext")
    s = unet_zoo_amd.create_model("unext_s", in_channels=1, num_classes=2, image_size=128)
    assert type(m) is UNext and type(s) is UNext_S
    assert s.patch_embed1.proj.in_channels == 1 and s.final_conv.out_channels == 2
    assert m.patch_embed1.img_size == (224, 224) and s.patch_embed1.img_size == (128, 128)


def test_parameter_counts():
    assert _count(unet_zoo_amd.create_model("unext")) == 14_305_345
    assert _count(unet_zoo_amd.create_model("unext_s")) == 2_961_057


def test_unext_s_drops_structure_kwargs_and_stray_kwargs_raise():
    s = unet_zoo_amd.create_model("unext_s", embed_dims=[32, 64, 96], num_heads=[1, 1, 1], depths=[1, 1, 1])
    assert _count(s) == 2_961_057
    m = unet_zoo_amd.create_model("unext", embed_dims=[64, 128, 160], num_heads=[1, 2, 4], depths=[2, 2, 2])
    assert _count(m) == 2_961_057       # UNext itself takes them
    with pytest.raises(TypeError):
        unet_zoo_amd.create_model("unext_s", not_an_option=1)
    with pytest.raises(TypeError):
        unet_zoo_amd.create_model("unext", not_an_option=1)


@pytest.mark.parametrize("name", ["unext", "unext_s"])
def test_seed0_state_dict_matches_the_reference_manifest(name):
    with open(os.path.join(GOLDEN, f"{name}_manifest.json")) as f:
        man = json.load(f)
    torch.manual_seed(0)
    sd = unet_zoo_amd.create_model(name, image_size=64).state_dict()
    assert list(sd.keys()) == [e[0] for e in man["entries"]]
    for k, shape, dtype, digest in man["entries"]:
        v = sd[k]
        assert list(v.shape) == shape and str(v.dtype) == "torch." + dtype
        assert _sha(v) == digest, f"seed-0 init of {k} differs from the reference"
    assert man["n_params"] == (14_305_345 if name == "unext" else 2_961_057)


def test_config_model_kwargs_build_unext(tmp_path):
    d = yaml.safe_load(CFG_YAML)
    d["general"]["working_dir"] = str(tmp_path)
    c = Config(d)
    assert c.MODELS_TO_TRAIN == ["unet", "unext", "unext_s"]
    for name, n in (("unext", 14_305_345), ("unext_s", 2_961_057)):
        m = unet_zoo_amd.create_model(name, **c.model_kwargs(name))
        assert _count(m) == n and m.patch_embed1.img_size == (512, 512)


def test_unsupported_options_are_refused():
    with pytest.raises(NotImplementedError, match="head size"):
        unet_zoo_amd.create_model("unext", embed_dims=[128, 160, 256], num_heads=[1, 1, 4])     # 160
    with pytest.raises(NotImplementedError, match="head size"):
        unet_zoo_amd.create_model("unext", embed_dims=[96, 160, 256], num_heads=[8, 2, 4])      # 12
    with pytest.raises(NotImplementedError, match="norm_layer"):
        unet_zoo_amd.create_model("unext_s", norm_layer=nn.BatchNorm1d)
    # head sizes 8 ... 128 in steps of 8 are accepted
    UNext(embed_dims=[8, 40, 128], num_heads=[1, 1, 1], depths=[1, 1, 1])


def test_training_with_dropout_is_refused_before_any_kernel():
    m = unet_zoo_amd.create_model("unext_s", drop_rate=0.1)
    with pytest.raises(NotImplementedError, match="drop"):
        m.emit(None, torch.zeros(1, 3, 64, 64))


@pytest.mark.parametrize("D", [12, 136, 0, 4])
def test_bad_sra_head_dim_is_rejected_without_a_gpu(D):
    lib = _lib.load()
    heads = 2
    C = heads * max(D, 8)
    d = _lib.SraDesc(_lib.UZ_BF16, 2, 64, 16, heads, D, 16, C, 2 * C, 2 * C, C, 0.125)
    assert lib.uz_sra_bwd_workspace_bytes(ctypes.byref(d)) == -1
    err = lib.uz_last_error_string()
    assert b"head_dim" in err and b"8" in err and b"128" in err


@pytest.mark.parametrize("D", [8, 40, 80, 128])
def test_new_sra_head_dims_pass_the_descriptor_check(D):
    lib = _lib.load()
    heads = 2
    C = heads * D
    d = _lib.SraDesc(_lib.UZ_BF16, 2, 64, 16, heads, D, 16, C, 2 * C, 2 * C, C, D ** -0.5)
    assert lib.uz_sra_bwd_workspace_bytes(ctypes.byref(d)) > 0


def test_token_maps_follow_the_reference_arithmetic_and_tiny_inputs_are_refused_before_any_kernel():
    m = unet_zoo_amd.create_model("unext_s")
    # k7 s4 p3, then k3 s2 p1 twice (Conv2d's floor): odd sizes are accepted, the reduction convolutions crop
    assert m.token_maps(100, 100) == [(25, 25), (13, 13), (7, 7)]
    assert m.token_maps(96, 160) == [(24, 40), (12, 20), (6, 10)]
    m.check_input_size(100, 100)
    m.check_input_size(29, 29)            # 8 x 8, 4 x 4, 2 x 2: the smallest maps with a full r x r window at every stage
    with pytest.raises(ValueError, match="reduction ratio"):
        m.emit(None, torch.zeros(1, 3, 20, 20))      # 5 x 5 tokens against r = 8: fails in the reference's Conv2d too
