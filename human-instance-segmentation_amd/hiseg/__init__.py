"""hiseg — MI355X-native ROI-hierarchical instance segmentation.

Drop-in for the RGB hierarchical path of PINTO0309/human-instance-segmentation
(HierarchicalRGBSegmentationModelWithFullImagePretrainedUNet + RefinedHierarchicalSegmentationHead
on a full-image EfficientNet-UNet, and the plain HierarchicalRGBSegmentationModel).  Module tree and state_dict keys follow the reference;
every forward runs on libhiseg (hand-written gfx950 HIP kernels, C ABI in include/hiseg.h).
"""
from .layers import (  # noqa: F401
    BoundaryRefinementModule, ChannelAttentionModule, ContourDetectionBranch, DistanceTransformDecoder, EnhancedUNet,
    ExtendedHierarchicalSegmentationHeadUNetV2, HierarchicalSegmentationHeadUNetV2, LayerNorm2d,
    PretrainedUNetGuidedSegmentationHead, RefinedHierarchicalSegmentationHead, ResidualBlock, RGBFeatureExtractor,
    SpatialAttentionModule)
from .effunet import EfficientNetUnet  # noqa: F401
from .model import (  # noqa: F401
    DynamicRoIAlign, HierarchicalRGBSegmentationModel, HierarchicalRGBSegmentationModelWithFullImagePretrainedUNet,
    PreTrainedPeopleSegmentationUNet,
    PreTrainedPeopleSegmentationUNetWrapper, RGBHierarchicalExportWrapper, StreamPipelinedExport,
    create_rgb_hierarchical_model)

from .losses import RefinedHierarchicalLoss, active_contour_term  # noqa: F401,E402
from .distance_loss import (  # noqa: F401,E402
    AdaptiveBoundaryLoss, DistanceAwareSegmentationLoss, create_distance_aware_loss)
from .optim import FusedAdamW, cosine_lr  # noqa: F401,E402
from .graphs import GraphedStep, GraphedBranchStep  # noqa: F401,E402
from .checkpoint import (  # noqa: F401,E402
    load_teacher_checkpoint, resume_distillation_checkpoint, resume_from_checkpoint, save_checkpoint,
    save_distillation_checkpoint)
from .data import GpuRoiBatchBuilder, resize_bilinear_pil  # noqa: F401,E402
from .augment import AugParams, RoiSafeAugmentation, augment_images  # noqa: F401,E402
from .metrics import (  # noqa: F401,E402
    SegmentationMetrics, calculate_confusion_matrix, calculate_detection_metrics, calculate_iou, evaluate_model,
)
from .distill import (  # noqa: F401,E402
    DistillationUNetWrapper, UNetDecoderOnly, UNetDistillationLoss, create_unet_distillation_model)
from .distill_eval import (  # noqa: F401,E402
    binary_seg_stats, distill_metrics_from_counts, evaluate_distillation, update_adaptive_distillation)
from .kd import (  # noqa: F401,E402
    DistillationLoss, DistillationModelWrapper, create_distilled_rgb_hierarchical_model)
from .postprocess import (  # noqa: F401,E402
    AdaptiveEdgeSmoothing, BilateralFilter, BinaryMaskBilateralFilter, BinaryMaskEdgeSmoothing,
    DirectionalEdgeSmoothing, EdgePreservingFilter, FastBilateralFilter, MorphologicalBilateralFilter,
    MultiClassEdgeSmoothing, OptimizedEdgeSmoothing, apply_edge_smoothing_to_masks)
from .compose import InstanceMapComposer, instance_colors  # noqa: F401,E402

__version__ = "0.2.0"


def set_compute_dtype(model, dtype):
    """Select the HIP compute precision of a model: torch.float32 (parity) or torch.bfloat16 (throughput)."""
    import torch
    if dtype not in (torch.float32, torch.bfloat16):
        raise TypeError(dtype)
    for m in model.modules():
        m.hiseg_dtype = dtype
    return model
