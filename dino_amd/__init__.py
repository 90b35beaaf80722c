"""dino_amd -- MI355X-native DINOSeg hot path (drop-in for ``from dt_segmentation import DINOSeg``)."""
import contextlib

from .augment import Augmenter, augment_table, draw_reference_augment  # noqa: F401
from .dinoseg import ClusterResult, ComponentsResult, DINOSeg, DiscoverResult, KnnResult, LabelPropagator, MaskCutResult, MemoryBank, NcutResult, PCAFitter, context_frames, dense_nll_loss, get_transforms, ncut_start, sample_indices, view_sizes, window_origins  # noqa: F401
from .pca import FeaturePCA, pca_solve  # noqa: F401
from .weights import VIT_B8, VIT_B16, VIT_S8, VIT_S16, ViTConfig, procedural_state_dict  # noqa: F401



def set_option(key: str, value: int) -> None:
    """Process-wide library switches (include/dinoseg.h: dinoseg_set_option), e.g. set_option("streams", 2): batches of >= 16
    frames run as two half-batches on two HIP streams."""
    from . import capi
    capi.check(capi.lib().dinoseg_set_option(key.encode(), int(value)))


def get_option(key: str) -> int:
    """The stored (normalised) value of one key of set_option (include/dinoseg.h: dinoseg_get_option)."""
    import ctypes
    from . import capi
    value = ctypes.c_int32()
    capi.check(capi.lib().dinoseg_get_option(key.encode(), ctypes.byref(value)))
    return value.value


def option_names() -> list:
    """Every key of set_option / get_option (include/dinoseg.h: dinoseg_option_name)."""
    from . import capi
    names = []
    while (name := capi.lib().dinoseg_option_name(len(names))) is not None:
        names.append(name.decode())
    return names


@contextlib.contextmanager
def options(**kw):
    """with options(mlp_fused=0, streams=1): ... -- set_option for each keyword; on exit (normal or by exception) every key of
    the library is back at its value from before the `with`, those the body changed with a bare set_option included.  Nests."""
    saved = {key: get_option(key) for key in option_names()}
    try:
        for key, value in kw.items():
            set_option(key, value)
        yield
    finally:
        for key, value in saved.items():
            if get_option(key) != value:
                set_option(key, value)


__all__ = ["DINOSeg", "ClusterResult", "NcutResult", "ComponentsResult", "DiscoverResult", "MaskCutResult", "LabelPropagator", "PCAFitter", "FeaturePCA", "pca_solve", "context_frames", "Augmenter", "augment_table", "draw_reference_augment", "dense_nll_loss", "get_transforms", "ncut_start", "sample_indices", "view_sizes", "window_origins", "ViTConfig", "VIT_S8", "VIT_B8", "VIT_S16", "VIT_B16", "procedural_state_dict", "set_option", "get_option", "options"]
