"""MI355X-native training hot path of EndoscopyDepthEstimation-Pytorch.

Drop-in ``nn.Module`` replacements (``models``, ``losses``), the reference's LR schedule
(``scheduler``), a fused clip+SGD optimizer (``optim``), one-collective data parallelism
(``distributed``), the training-iteration glue and validation pass (``train_step``), the display panels (``display``) and evaluate.py's test
phase (``evaluate``), the fusion of its posed depth maps into one surface (``fusion``), a triangle mesh such as the CT model seen from a frame's camera (``mesh``) and the similarity registration of its point
clouds to a model (``registration``), all on hand-written HIP kernels
for gfx950 behind the C ABI of ``include/endo_hip.h``.  See DESIGN.md / INTEGRATION.md.

The directory name carries a hyphen, so import it with
``importlib.import_module("endoscopydepthestimation-pytorch_amd")`` or ``import endo_amd``.
"""

from . import _lib, augment, dataset, display, distributed, evaluate, fusion, losses, mesh, models, optim, reader, registration, scatter, scheduler, synthetic, train_step, utils  # noqa: F401
from .models import FCDenseNet57, DepthScalingLayer, DepthWarpingLayer, FlowfromDepthLayer  # noqa: F401
from .models import images_warping, _bilinear_interpolate, _warp_coordinate_generate  # noqa: F401
from .losses import SparseMaskedL1Loss, NormalizedDistanceLoss, ScaleInvariantLoss, AbsRelError, Threshold  # noqa: F401
from .losses import (NormalizedWeightedMaskedL2Loss, SparseMaskedL1LossDisplay, MaskedL1Loss, NormalizedL2Loss, NormalizedL1Loss,  # noqa: F401
                     MaskedScaleInvariantLoss, PhotometricLoss)
