# -*- coding: utf-8 -*-
"""emsanet_amd: MI355X-native EMSANet forward/backward engine (hand-written HIP, gfx950)."""
from .args import default_args, full_args          # noqa: F401
from .data import DatasetConfig, nyuv2_config      # noqa: F401


def __getattr__(name):
    # lazy: importing the model requires torch; the C-ABI library is loaded on first use
    if name == 'EMSANet':
        from .model import EMSANet
        return EMSANet
    if name == 'get_decoders':
        from .decoder import get_decoders
        return get_decoders
    if name in ('MeanIntersectionOverUnion', 'PanopticQuality', 'panoptic_targets', 'SceneAccuracy',
                'MeanAbsoluteAngularError', 'MeanAbsoluteNormalError'):
        from . import metrics
        return getattr(metrics, name)
    if name in ('TrainingTargetGenerator', 'orientation_table'):
        from . import targets
        return getattr(targets, name)
    if name == 'NormalLoss':
        from .loss import NormalLoss
        return NormalLoss
    if name == 'NormalPostprocessing':
        from .postprocessing import NormalPostprocessing
        return NormalPostprocessing
    if name == 'ValidationEvaluator':
        from .evaluation import ValidationEvaluator
        return ValidationEvaluator
    if name == 'TrainingAugmenter':
        from .augment import TrainingAugmenter
        return TrainingAugmenter
    if name in ('InferenceOutputPacker', 'write_mapping_output'):
        from . import export
        return getattr(export, name)
    if name in ('PngEncoder', 'write_scannet_output', 'PngDecoder', 'PngFiles', 'PngDecodeError',
                'png_info'):
        from . import png
        return getattr(png, name)
    raise AttributeError(name)
