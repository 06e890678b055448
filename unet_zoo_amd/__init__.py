"""unet_zoo_amd — MI355X-native (gfx950) engine for the unet_zoo encoder/decoder hot path.

Drop-in surface: ``create_model`` / ``list_models`` as in ``unet_zoo`` (reference
unet_zoo/__init__.py:1).  The arithmetic runs in hand-written HIP kernels behind the C ABI of
``libunetzoo_hip.so`` (include/unetzoo_hip.h); there is no CPU or PyTorch fallback.
"""
from .models import create_model, list_models, get_model_config, hip_models
from .graph import set_default_dtype, get_default_dtype
from .step import GraphedStep
from .evalstep import GraphedEval
from .loss import MulticlassLoss, RegionLoss
from .boundary import BoundaryLoss
from .lovasz import LovaszLoss
from .hardpixel import HardPixelLoss
from .cldice import ClDiceLoss
from .augment import GpuAugment
from .patches import PatchSampler
from .schedule import LrSchedule
from .surface import SurfaceMetrics
from .confusion import ConfusionMetrics
from .postprocess import MaskPostprocess
from .predict import GraphedPredict
from .tiled import SlidingWindowPredict
from .config import Config, load_config

__version__ = "0.1.0"
__all__ = ["create_model", "list_models", "get_model_config", "hip_models", "set_default_dtype",
           "get_default_dtype", "GraphedStep", "GraphedEval", "RegionLoss", "MulticlassLoss", "BoundaryLoss", "LovaszLoss", "ClDiceLoss", "HardPixelLoss", "GpuAugment", "PatchSampler", "LrSchedule", "SurfaceMetrics", "ConfusionMetrics",
           "MaskPostprocess", "GraphedPredict", "SlidingWindowPredict",
           "Config", "load_config"]
