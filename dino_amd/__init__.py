"""dino_amd -- MI355X-native DINOSeg hot path (drop-in for ``from dt_segmentation import DINOSeg``)."""
from .augment import Augmenter, augment_table, draw_reference_augment  # noqa: F401
from .dinoseg import ClusterResult, ComponentsResult, DINOSeg, DiscoverResult, LabelPropagator, MaskCutResult, NcutResult, context_frames, dense_nll_loss, get_transforms, ncut_start, sample_indices, view_sizes, window_origins  # noqa: F401
from .weights import VIT_B8, VIT_B16, VIT_S8, VIT_S16, ViTConfig, procedural_state_dict  # noqa: F401



def set_option(key: str, value: int) -> None:
    """Process-wide library switches (include/dinoseg.h: dinoseg_set_option), e.g. set_option("streams", 2): batches of >= 16
    frames run as two half-batches on two HIP streams."""
    from . import capi
    capi.check(capi.lib().dinoseg_set_option(key.encode(), int(value)))


__all__ = ["DINOSeg", "ClusterResult", "NcutResult", "ComponentsResult", "DiscoverResult", "MaskCutResult", "LabelPropagator", "context_frames", "Augmenter", "augment_table", "draw_reference_augment", "dense_nll_loss", "get_transforms", "ncut_start", "sample_indices", "view_sizes", "window_origins", "ViTConfig", "VIT_S8", "VIT_B8", "VIT_S16", "VIT_B16", "procedural_state_dict", "set_option"]
