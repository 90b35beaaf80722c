"""The device-free half of ``DINOSeg``'s pixel-resolution modes: everything that decides or refuses from shapes and the patch
size alone.  Nothing here touches a device or a native handle (``window_origins`` calls a host-only entry of the library), so
every ``ValueError`` of a pixel-resolution call is raised before the model asks for a GPU.  ``dinoseg.py`` holds the other
half: the runners that allocate and launch.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import capi

ENSEMBLE_MAX_VIEWS = 12        # include/dinoseg.h: dinoseg_op_upsample_ensemble takes 1 .. 12 views
WINDOW_MAX_COVERAGE = 4        # include/dinoseg.h: dinoseg_op_window_merge takes at most 4 windows over a pixel row / column


def view_sizes(H: int, W: int, scales, patch: int) -> List[Tuple[int, int]]:
    """The frame sizes of a multi-scale protocol: per scale s the H x W frame scaled by s and rounded to the nearest multiple of
    the patch (halves up, at least one patch): ``H_k = patch * max(1, floor(H * s / patch + 0.5))``, the same for W."""
    def one(v, s):
        return patch * max(1, int(math.floor(v * s / patch + 0.5)))
    return [(one(H, float(s)), one(W, float(s))) for s in scales]


def window_origins(L: int, window: int, stride: int) -> List[int]:
    """The origins of the sliding windows along one axis (mmsegmentation's ``slide_inference``): frame side ``L``, window
    ``1 <= window <= L``, stride ``>= 1``; ``g = max(L - window + stride - 1, 0) // stride + 1`` windows at ``max(min(i * stride +
    window, L) - window, 0)`` -- the last one is shifted back to end at ``L``.  The rule lives in the library
    (``dinoseg_window_origins``, host only: no device needed)."""
    L, window, stride = int(L), int(window), int(stride)
    lib = capi.lib()
    g = lib.dinoseg_window_origins(L, window, stride, None, 0)
    if g < 1:
        raise ValueError(f"bad window rule: frame side {L}, window {window}, stride {stride} (1 <= window <= frame side, stride >= 1)")
    out = (C.c_int32 * g)()
    if lib.dinoseg_window_origins(L, window, stride, out, g) != g:
        raise capi.DinosegError(capi.last_error())
    return list(out)


def _pair(v, what: str) -> Tuple[int, int]:
    try:
        a, b = (v, v) if isinstance(v, (int, np.integer)) else v
        return int(a), int(b)
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be an integer or a pair of integers, got {v!r}") from None


def guided_params(guided=True, radius=2, sigma_spatial=1.0, sigma_range=0.1):
    """The validated (radius, sigma_spatial, sigma_range) of an image-guided upsample (``DINOSeg.segment_guided``): ``guided`` is
    ``True`` (the defaults) or a dict with any of the three keys.  The ranges are the library's (include/dinoseg.h,
    dinoseg_op_upsample_guided): radius 0..3 cells, sigma_spatial in [0.5, 16] cells, sigma_range in [1e-3, 1e3] of the 0..255
    range.  Every ``ValueError`` is raised here, before any device use."""
    if isinstance(guided, dict):
        unknown = set(guided) - {"radius", "sigma_spatial", "sigma_range"}
        if unknown:
            raise ValueError(f"guided takes radius / sigma_spatial / sigma_range, got {sorted(unknown)}")
        radius = guided.get("radius", radius)
        sigma_spatial = guided.get("sigma_spatial", sigma_spatial)
        sigma_range = guided.get("sigma_range", sigma_range)
    elif guided is not True:
        raise ValueError(f"guided must be True or a dict of radius / sigma_spatial / sigma_range, got {guided!r}")
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= int(radius) <= 3:
        raise ValueError(f"radius must be an integer in 0..3, got {radius!r}")
    sigma_spatial, sigma_range = float(sigma_spatial), float(sigma_range)
    if not (math.isfinite(sigma_spatial) and 0.5 <= sigma_spatial <= 16.0):
        raise ValueError(f"sigma_spatial must be in [0.5, 16] (cells), got {sigma_spatial}")
    if not (math.isfinite(sigma_range) and 1e-3 <= sigma_range <= 1e3):
        raise ValueError(f"sigma_range must be in [1e-3, 1e3] (of the 0..255 range), got {sigma_range}")
    return int(radius), sigma_spatial, sigma_range


def _axis_coverage(origins: List[int], window: int) -> int:
    """The most windows over one pixel of the axis (attained at a window's first pixel)."""
    most, i = 1, 0
    for j, oj in enumerate(origins):
        while origins[i] + window <= oj:
            i += 1
        most = max(most, j - i + 1)
    return most


def resolution_message(patch: int) -> str:
    # patch 8: the reference's text (pl_torch_modules.py:271-272), byte for byte
    return "Resolution should be a multiple of 16." if patch == 16 else "Resolution should be a multiple of 8."


def frame_layout(x: torch.Tensor, patch: int, multiple: bool = False, one_patch: bool = False, non_empty: bool = False,
                 u8_only: bool = False) -> Tuple[int, int, int, int]:
    """The two frame layouts, uint8 [B,H,W,3] and fp32 [B,3,H,W] (any other dtype is read as the second): (input kind, B, H, W).
    ``multiple``: H and W are multiples of the patch; ``one_patch``: at least one patch each; ``non_empty``: B >= 1;
    ``u8_only``: only the first layout is taken (``forward_frames``)."""
    u8 = x.dtype == torch.uint8
    if u8_only and not (u8 and x.dim() == 4 and x.shape[3] == 3):
        raise ValueError(f"expected uint8 [B,H,W,3], got {x.dtype} {tuple(x.shape)}")
    if u8:
        if x.dim() != 4 or x.shape[3] != 3:
            raise ValueError(f"expected uint8 [B,H,W,3], got {tuple(x.shape)}")
        kind, B, H, W = capi.INPUT_U8_HWC, x.shape[0], x.shape[1], x.shape[2]
    else:
        if x.dim() != 4 or x.shape[1] != 3:
            raise ValueError(f"expected [B,3,H,W], got {tuple(x.shape)}")
        kind, B, H, W = capi.INPUT_F32_CHW, x.shape[0], x.shape[2], x.shape[3]
    if (multiple and (H % patch != 0 or W % patch != 0)) or (one_patch and (H < patch or W < patch)):
        raise ValueError(resolution_message(patch))
    if non_empty and B < 1:
        raise ValueError("empty batch")
    return kind, B, H, W


def label_size(y: torch.Tensor, B: int, own: Optional[Tuple[int, int]] = None) -> Tuple[int, int]:
    """The (OH, OW) of pixel labels [B, OH, OW]; with ``own`` (sliding windows) they must have that size, the frames'."""
    if y.dim() != 3 or y.shape[0] != B or (own is not None and tuple(y.shape[1:]) != tuple(own)):
        want = "OH, OW]" if own is None else f"{own[0]}, {own[1]}] (the frames' own size)"
        raise ValueError(f"expected pixel labels [B={B}, {want}, got {tuple(y.shape)}")
    return int(y.shape[1]), int(y.shape[2])


def out_size(size, default) -> Tuple[int, int]:
    OH, OW = (int(v) for v in (default if size is None else size))
    return OH, OW


def window_plan(patch: int, H: int, W: int, window, stride):
    """The window and stride of a sliding-window call on H x W frames, per axis: ((wh, ww), (sh, sw), (gh, gw)).  Every
    ``ValueError`` of the protocol is raised here, before any device use."""
    p = patch
    if H < p or W < p:
        raise ValueError(f"frames of {H}x{W} are smaller than one {p}x{p} patch")
    win, out_s, grid = list(_pair(window, "window")), [], []
    st = (None, None) if stride is None else _pair(stride, "stride")
    for axis, L in enumerate((H, W)):
        w, name = win[axis], ("vertical", "horizontal")[axis]
        if w < 1:
            raise ValueError(f"window must be positive, got {tuple(_pair(window, 'window'))}")
        if w % p != 0:
            raise ValueError(f"{name} window {w} is not a multiple of the patch ({p})")
        w = min(w, (L // p) * p)                    # clamped to the largest patch multiple inside the frame
        s = (2 * w) // 3 if st[axis] is None else st[axis]
        if s < 1:
            raise ValueError(f"stride must be positive, got {tuple(st)}")
        origins = window_origins(L, w, s)
        cov = _axis_coverage(origins, w)
        if cov > WINDOW_MAX_COVERAGE:
            raise ValueError(f"{name} coverage {cov}: window {w} at stride {s} puts {cov} windows over one pixel "
                             f"{'row' if axis == 0 else 'column'} (at most {WINDOW_MAX_COVERAGE} per axis)")
        win[axis] = w
        out_s.append(s)
        grid.append(len(origins))
    return tuple(win), tuple(out_s), tuple(grid)


def guide_plan(patch: int, x: torch.Tensor, guide, size):
    """The shape checks of ``segment_guided`` without a device: (kind, B, H, W, OH, OW)."""
    kind, B, H, W = frame_layout(x, patch, multiple=True, one_patch=True, non_empty=True)
    if guide is None:
        if kind != capi.INPUT_U8_HWC:
            raise ValueError("fp32 frames carry no image to guide by: pass guide=uint8 [B,OH,OW,3] (or uint8 frames)")
        OH, OW = out_size(size, (H, W))
    else:
        if not isinstance(guide, torch.Tensor) or guide.dtype != torch.uint8 or guide.dim() != 4 or guide.shape[3] != 3:
            raise ValueError(f"expected a uint8 guide [B,OH,OW,3], got {getattr(guide, 'dtype', type(guide).__name__)} "
                             f"{tuple(getattr(guide, 'shape', ()))}")
        if guide.shape[0] != B:
            raise ValueError(f"the guide has {guide.shape[0]} frames, the batch {B}")
        OH, OW = out_size(size, guide.shape[1:3])
        if (OH, OW) != tuple(guide.shape[1:3]):
            raise ValueError(f"size {(OH, OW)} differs from the guide's {tuple(guide.shape[1:3])} (the guide is at the output's size)")
    if OH < H // patch or OW < W // patch:
        raise ValueError(f"size {(OH, OW)} is smaller than the patch grid {(H // patch, W // patch)}")
    return kind, B, H, W, OH, OW


REFINE_DILATIONS = (1, 2, 4, 8, 12, 24)     # PAMR's
REFINE_MAX_SIDE = 1 << 14


def refine_params(gain=1.0, iters=10, dilations=REFINE_DILATIONS, sigma=0.1):
    """The validated (gain, iters, dilations, sigma) of a refinement (include/dinoseg.h, dinoseg_op_refine_iterate): gain positive
    and finite, iters an integer in 0..64, 1 to 6 strictly ascending integer dilations in 1..24, sigma in [1e-3, 1e3]."""
    try:
        gain, sigma = float(gain), float(sigma)
    except (TypeError, ValueError):
        raise ValueError(f"gain and sigma must be numbers, got {gain!r} and {sigma!r}") from None
    with np.errstate(over="ignore", under="ignore"):
        gain32 = float(np.float32(gain))            # (the library multiplies by the fp32 value)
    if not (math.isfinite(gain) and gain > 0.0 and math.isfinite(gain32) and gain32 > 0.0):
        raise ValueError(f"gain must be positive and finite (in fp32 too), got {gain}")
    if not (math.isfinite(sigma) and 1e-3 <= sigma <= 1e3):
        raise ValueError(f"sigma must be in [1e-3, 1e3], got {sigma}")
    if isinstance(iters, bool) or not isinstance(iters, (int, np.integer)) or not 0 <= int(iters) <= 64:
        raise ValueError(f"iters must be an integer in 0..64, got {iters!r}")
    try:
        dil = tuple(dilations)
    except TypeError:
        raise ValueError(f"dilations must be a sequence of integers, got {dilations!r}") from None
    if not 1 <= len(dil) <= 6:
        raise ValueError(f"dilations takes 1 to 6 entries, got {len(dil)}")
    if any(isinstance(d, bool) or not isinstance(d, (int, np.integer)) or not 1 <= int(d) <= 24 for d in dil):
        raise ValueError(f"every dilation must be an integer in 1..24, got {dil}")
    dil = tuple(int(d) for d in dil)
    if any(b <= a for a, b in zip(dil, dil[1:])):
        raise ValueError(f"dilations must ascend strictly, got {dil}")
    return gain, int(iters), dil, sigma


def refine_plan(seed, guide, n_classes=None, grid=None, gain=1.0, iters=10, dilations=REFINE_DILATIONS, sigma=0.1):
    """The checks of ``DINOSeg.refine`` without a device: (kind, B, C, OH, OW, hp, wp, gain, iters, dilations, sigma).  kind 0: an
    integer label map [B, OH, OW] at the guide's size with ``n_classes``; kind 1: fp32 scores [B, n, C] with ``grid=(hp, wp)``,
    n == hp * wp, no larger than the guide.  Every ``ValueError`` is raised here, before any device use."""
    if not isinstance(guide, torch.Tensor) or guide.dtype != torch.uint8 or guide.dim() != 4 or guide.shape[3] != 3:
        raise ValueError(f"expected a uint8 guide [B,OH,OW,3], got {getattr(guide, 'dtype', type(guide).__name__)} "
                         f"{tuple(getattr(guide, 'shape', ()))}")
    B, OH, OW = (int(v) for v in guide.shape[:3])
    if B < 1:
        raise ValueError("empty batch")
    if not (1 <= OH <= REFINE_MAX_SIDE and 1 <= OW <= REFINE_MAX_SIDE):
        raise ValueError(f"the guide's size {(OH, OW)} must be in 1..{REFINE_MAX_SIDE} per side")
    if not isinstance(seed, torch.Tensor):
        raise ValueError(f"expected a seed tensor, got {type(seed).__name__}")
    hp = wp = 0
    if seed.dtype in (torch.int8, torch.int16, torch.int32, torch.int64, torch.uint8):
        kind = 0
        if seed.dim() != 3 or tuple(seed.shape) != (B, OH, OW):
            raise ValueError(f"expected seed labels [B={B}, {OH}, {OW}] (the guide's size), got {tuple(seed.shape)}")
        if n_classes is None:
            raise ValueError("a label seed needs n_classes")
        if grid is not None:
            raise ValueError("grid belongs to a scores seed; a label seed is at the guide's size")
        C = n_classes
    elif seed.dtype == torch.float32:
        kind = 1
        if seed.dim() != 3 or seed.shape[0] != B:
            raise ValueError(f"expected seed scores [B={B}, n, C], got {tuple(seed.shape)}")
        if grid is None:
            raise ValueError("a scores seed needs grid=(hp, wp)")
        hp, wp = _pair(grid, "grid")
        if hp < 1 or wp < 1 or hp * wp != seed.shape[1]:
            raise ValueError(f"grid {(hp, wp)} does not hold the seed's {seed.shape[1]} rows")
        if OH < hp or OW < wp:
            raise ValueError(f"the guide's size {(OH, OW)} is smaller than the grid {(hp, wp)}")
        C = int(seed.shape[2])
        if n_classes is not None and int(n_classes) != C:
            raise ValueError(f"n_classes={n_classes} differs from the seed's {C} columns")
    else:
        raise ValueError(f"expected an integer label map [B,OH,OW] or fp32 scores [B,n,C], got {seed.dtype}")
    if isinstance(C, bool) or not isinstance(C, (int, np.integer)) or not 1 <= int(C) <= 256:
        raise ValueError(f"n_classes must be an integer in 1..256, got {C!r}")
    gain, iters, dil, sigma = refine_params(gain, iters, dilations, sigma)
    return kind, B, int(C), OH, OW, hp, wp, gain, iters, dil, sigma


def multiscale_plan(patch: int, H: int, W: int, scales, flip: bool, size):
    """The views of ``segment_multiscale`` on H x W frames: ([(H_k, W_k, flip_k)] scale-major, the unflipped view first; their
    count K; the output's (OH, OW))."""
    scales = tuple(float(s) for s in scales)
    K = len(scales) * (2 if flip else 1)
    if not 1 <= K <= ENSEMBLE_MAX_VIEWS:
        raise ValueError(f"{len(scales)} scales{' with flip' if flip else ''} are {K} views; the ensemble takes 1 to {ENSEMBLE_MAX_VIEWS}")
    if any(not (s > 0.0 and math.isfinite(s)) for s in scales):
        raise ValueError(f"scales must be positive, got {scales}")
    OH, OW = out_size(size, (H, W))
    views = [(Hk, Wk, f) for Hk, Wk in view_sizes(H, W, scales, patch) for f in ((0, 1) if flip else (0,))]
    for Hk, Wk, _ in views:
        if Hk // patch > OH or Wk // patch > OW:
            raise ValueError(f"the {Hk}x{Wk} view's grid {Hk // patch}x{Wk // patch} exceeds the output size {OH}x{OW} "
                             "(upsampling and identity only)")
    return views, K, (OH, OW)


class DenseMode(NamedTuple):
    """What ``predict_dense`` / ``validation_step_dense`` were asked for.  ``args`` by ``kind``: "bilinear" (), "multiscale"
    (scales, flip), "windows" (window, stride: checked against the frames by ``window_plan``), "guided" the validated (radius,
    sigma_spatial, sigma_range)."""
    kind: str
    args: tuple = ()


def dense_mode(scales=None, flip: bool = False, window=None, stride=None, guided=None) -> DenseMode:
    """The one mode the five keywords of ``predict_dense`` / ``validation_step_dense`` select, or the ``ValueError`` of a
    combination that is not one."""
    if guided is not None:
        if window is not None or scales is not None:
            raise ValueError("guided cannot be combined with window or scales")
        return DenseMode("guided", guided_params(guided))
    if window is not None:
        if scales is not None:
            raise ValueError("window and scales cannot be combined")
        return DenseMode("windows", (window, stride))
    if scales is not None:
        return DenseMode("multiscale", (tuple(scales), bool(flip)))
    return DenseMode("bilinear")


# ---- video label propagation (include/dinoseg.h: dinoseg_op_propagate) ----
PROPAGATE_MAX_CONTEXT = 16     # context frames of one target frame: frame 0 and up to 15 queued ones
PROPAGATE_MAX_K = 16
PROPAGATE_MAX_CLASSES = 256


def context_frames(t: int, n_context: int) -> List[int]:
    """The context list of target frame ``t >= 1``: frame 0 first, then the last ``min(t - 1, n_context)`` frames before ``t``,
    oldest first (frame 0 never enters the queue): t = 1 -> [0]; t = 2 -> [0, 1]; t = 9, n_context = 7 -> [0, 2 .. 8]."""
    t, n_context = int(t), int(n_context)
    if t < 1 or not 0 <= n_context <= PROPAGATE_MAX_CONTEXT - 1:
        raise ValueError(f"context_frames: target frame {t} (>= 1), n_context {n_context} (0 .. {PROPAGATE_MAX_CONTEXT - 1})")
    return [0] + list(range(max(1, t - n_context), t))


class PropagatePlan(NamedTuple):
    """What a propagation call was asked for, validated: the frames' layout, the patch grid, the seed's kind ("labels": integer
    pixel labels [OH0, OW0]; "soft": fp32 [n, C]), the rule's parameters and the output size."""
    kind: int
    T: int
    H: int
    W: int
    hp: int
    wp: int
    C: int
    seed: str
    n_context: int
    radius: int
    topk: int
    temperature: float
    OH: int
    OW: int
    chunk: int


def _int_in(v, lo: int, hi: int, what: str) -> int:
    if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not lo <= int(v) <= hi:
        raise ValueError(f"{what} must be an integer in {lo}..{hi}, got {v!r}")
    return int(v)


def propagate_plan(patch: int, frames: torch.Tensor, first, n_classes=None, n_context=7, radius=12, topk=5, temperature=0.1,
                   size=None, chunk=32) -> PropagatePlan:
    """The shape and parameter checks of ``DINOSeg.propagate`` / ``LabelPropagator`` without a device.  ``frames`` is the clip
    (uint8 [T,H,W,3] or fp32 [T,3,H,W]; the propagator passes its first frame as a clip of one); ``first`` the seed of frame 0:
    integer pixel labels [OH0, OW0] at least as large as the patch grid (``n_classes`` required) or a soft fp32 [n, C].
    ``radius=None`` is the whole frame.  Every ``ValueError`` is raised here, before any device use."""
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f"expected the clip as a tensor, uint8 [T,H,W,3] or fp32 [T,3,H,W], got {type(frames).__name__}")
    kind, T, H, W = frame_layout(frames, patch, multiple=True, one_patch=True, non_empty=True)
    hp, wp = H // patch, W // patch
    n = hp * wp
    n_context = _int_in(n_context, 0, PROPAGATE_MAX_CONTEXT - 1, "n_context")
    topk = _int_in(topk, 1, PROPAGATE_MAX_K, "topk")
    chunk = _int_in(chunk, 1, 1 << 20, "chunk")
    if radius is None:
        radius = max(hp, wp)
    radius = _int_in(radius, 0, 1 << 30, "radius")
    try:
        temperature = float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"temperature must be a positive number, got {temperature!r}") from None
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"temperature must be finite and positive, got {temperature}")
    if n_classes is not None:
        n_classes = _int_in(n_classes, 1, PROPAGATE_MAX_CLASSES, "n_classes")
    if not isinstance(first, torch.Tensor) or first.dim() != 2 or first.dtype == torch.bool:
        raise ValueError("first must be integer pixel labels [OH0, OW0] or a soft fp32 seed [n, C], got "
                         f"{getattr(first, 'dtype', type(first).__name__)} {tuple(getattr(first, 'shape', ()))}")
    if first.is_floating_point():
        if first.shape[0] != n or not 1 <= first.shape[1] <= PROPAGATE_MAX_CLASSES:
            raise ValueError(f"a soft seed is [n = {n}, C] with 1 <= C <= {PROPAGATE_MAX_CLASSES}, got {tuple(first.shape)}")
        C, seed = int(first.shape[1]), "soft"
        if n_classes is not None and n_classes != C:
            raise ValueError(f"n_classes = {n_classes} differs from the soft seed's {C} columns")
    else:
        if n_classes is None:
            raise ValueError("integer pixel labels need n_classes")
        if first.shape[0] < hp or first.shape[1] < wp:
            raise ValueError(f"pixel labels of {tuple(first.shape)} are smaller than the patch grid {(hp, wp)}")
        C, seed = n_classes, "labels"
    try:
        OH, OW = out_size(size, (H, W))
    except (TypeError, ValueError):
        raise ValueError(f"size must be a pair (OH, OW), got {size!r}") from None
    if OH < hp or OW < wp:
        raise ValueError(f"size {(OH, OW)} is smaller than the patch grid {(hp, wp)}")
    return PropagatePlan(kind, int(T), int(H), int(W), hp, wp, C, seed, n_context, radius, topk, temperature, OH, OW, chunk)


# ---- few-shot segmentation: k-NN label retrieval from a memory bank (include/dinoseg.h: dinoseg_op_knn_labels) ----
KNN_MAX_K = 16
KNN_MAX_ROWS = 1 << 24


class KnnPlan(NamedTuple):
    """What a ``segment_knn`` call was asked for, validated: the frames' layout, the patch grid, the bank's live rows and classes,
    the rule's parameters and the output size."""
    kind: int
    B: int
    H: int
    W: int
    hp: int
    wp: int
    M: int
    C: int
    topk: int
    temperature: float
    OH: int
    OW: int
    chunk: int
    n_blocks: int


def _temperature(temperature) -> float:
    try:
        temperature = float(temperature)
    except (TypeError, ValueError):
        raise ValueError(f"temperature must be a positive number, got {temperature!r}") from None
    if not (math.isfinite(temperature) and temperature > 0.0):
        raise ValueError(f"temperature must be finite and positive, got {temperature}")
    return temperature


def knn_plan(patch: int, embed_dim: int, x: torch.Tensor, bank_size: int, bank_dim: int, bank_classes: int, bank_blocks: int,
             n_blocks=None, topk=10, temperature=0.1, size=None, chunk=32, project=None) -> KnnPlan:
    """The shape and parameter checks of ``DINOSeg.segment_knn`` without a device.  ``x`` is the batch (uint8 [B,H,W,3] or fp32
    [B,3,H,W], H and W multiples of the patch size); ``bank_size``, ``bank_dim``, ``bank_classes`` and ``bank_blocks`` are the
    bank's live rows, row width, classes and the ``n_blocks`` its features were taken after; ``n_blocks=None`` is the bank's.
    ``project`` is the bank's ``FeaturePCA`` when it has one: its rows then have the projection's width, not the model's.
    Every ``ValueError`` is raised here, before any device use."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"expected the frames as a tensor, uint8 [B,H,W,3] or fp32 [B,3,H,W], got {type(x).__name__}")
    kind, B, H, W = frame_layout(x, patch, multiple=True, one_patch=True, non_empty=True)
    hp, wp = H // patch, W // patch
    topk = _int_in(topk, 1, KNN_MAX_K, "topk")
    chunk = _int_in(chunk, 1, 1 << 20, "chunk")
    temperature = _temperature(temperature)
    if int(bank_size) < 1:
        raise ValueError("the memory bank is empty: add labelled frames first")
    if project is not None:
        pca_projection(project, embed_dim, "the memory bank's projection", bank=True, blocks=bank_blocks)
        if int(bank_dim) != project.q:
            raise ValueError(f"the memory bank holds rows of width {bank_dim}, its projection has {project.q} components")
    elif int(bank_dim) != int(embed_dim):
        raise ValueError(f"the memory bank holds rows of width {bank_dim}, the model's embed_dim is {embed_dim}")
    if n_blocks is not None and int(n_blocks) != int(bank_blocks):
        raise ValueError(f"the memory bank was filled with n_blocks = {bank_blocks}, the call asks for n_blocks = {n_blocks}")
    try:
        OH, OW = out_size(size, (H, W))
    except (TypeError, ValueError):
        raise ValueError(f"size must be a pair (OH, OW), got {size!r}") from None
    if OH < hp or OW < wp:
        raise ValueError(f"size {(OH, OW)} is smaller than the patch grid {(hp, wp)}")
    return KnnPlan(kind, int(B), int(H), int(W), hp, wp, int(bank_size), int(bank_classes), topk, temperature, OH, OW, chunk,
                   int(bank_blocks))


class BankAddPlan(NamedTuple):
    """What a ``MemoryBank.add`` call was asked for, validated: the frames' layout, the patch grid, the labels' size and kind
    (0 = uint8, 1 = int64, as ``dinoseg_op_label_cells``), the cells kept per frame and the rows the call adds."""
    kind: int
    B: int
    hp: int
    wp: int
    OH: int
    OW: int
    mask_kind: int
    per_frame: int
    rows: int
    seed: int


def bank_add_plan(patch: int, frames: torch.Tensor, labels: torch.Tensor, per_frame=None, seed=0, room: int = KNN_MAX_ROWS) -> BankAddPlan:
    """The checks of ``MemoryBank.add`` without a device: ``frames`` as in ``knn_plan``, ``labels`` integer [B, OH, OW] at least as
    large as the patch grid, ``per_frame`` the cells kept per frame (``None``: all), ``room`` the rows the bank can still take."""
    if not isinstance(frames, torch.Tensor):
        raise ValueError(f"expected the frames as a tensor, uint8 [B,H,W,3] or fp32 [B,3,H,W], got {type(frames).__name__}")
    kind, B, H, W = frame_layout(frames, patch, multiple=True, one_patch=True, non_empty=True)
    hp, wp = H // patch, W // patch
    if not isinstance(labels, torch.Tensor) or labels.is_floating_point() or labels.dtype == torch.bool:
        raise ValueError(f"labels must be integer pixel labels [B, OH, OW], got {getattr(labels, 'dtype', type(labels).__name__)}")
    OH, OW = label_size(labels, B)
    if OH < hp or OW < wp:
        raise ValueError(f"pixel labels of {(OH, OW)} are smaller than the patch grid {(hp, wp)}")
    per_frame = hp * wp if per_frame is None else _int_in(per_frame, 1, hp * wp, "per_frame")
    seed = _int_in(seed, -(1 << 62), 1 << 62, "seed")
    rows = int(B) * per_frame
    if rows > room:
        raise ValueError(f"the call adds {rows} rows, the memory bank has room for {room}")
    return BankAddPlan(kind, int(B), hp, wp, OH, OW, 0 if labels.dtype == torch.uint8 else 1, per_frame, rows, seed)


# ---- unsupervised segmentation: spherical k-means over patch features (include/dinoseg.h: dinoseg_op_kmeans_assign) ----
KMEANS_MAX_K = 256             # the class limit of dinoseg_op_upsample_argmax


class KMeansPlan(NamedTuple):
    """What a clustering call was asked for, validated: the frames' layout, the patch grid, the number of points N = B n, the rule's
    parameters, how the centroids start ("sample": K distinct points drawn on the host; "rows": the caller's fp32 [k, D]) and the
    output size."""
    kind: int
    B: int
    H: int
    W: int
    hp: int
    wp: int
    N: int
    k: int
    iters: int
    init: str
    seed: int
    n_init: int
    OH: int
    OW: int
    chunk: int


def sample_indices(N: int, k: int, seed: int) -> torch.Tensor:
    """The K distinct point indices of ``init="sample"``: the head of a seeded host permutation (the library has no device random
    numbers), int64 [k]."""
    N, k = int(N), int(k)
    if not 1 <= k <= N:
        raise ValueError(f"init='sample' draws k = {k} distinct points out of N = {N}")
    return torch.randperm(N, generator=torch.Generator().manual_seed(int(seed)))[:k]


def _centroid_rows(rows, k, embed_dim: int, what: str) -> int:
    if not isinstance(rows, torch.Tensor) or rows.dim() != 2 or rows.dtype != torch.float32 or rows.shape[1] != embed_dim or \
            not 1 <= rows.shape[0] <= KMEANS_MAX_K or (k is not None and rows.shape[0] != k):
        want = "1.." + str(KMEANS_MAX_K) if k is None else str(k)
        raise ValueError(f"{what} must be {'the string sample or ' if what == 'init' else ''}fp32 rows [{want}, {embed_dim}], got "
                         f"{getattr(rows, 'dtype', type(rows).__name__)} {tuple(getattr(rows, 'shape', ()))}")
    return int(rows.shape[0])


def kmeans_plan(patch: int, embed_dim: int, x: torch.Tensor, k, iters=10, init="sample", seed=0, n_init=1, size=None,
                chunk=32) -> KMeansPlan:
    """The shape and parameter checks of ``DINOSeg.cluster`` / ``DINOSeg.assign_clusters`` without a device.  ``x`` is the batch or clip
    (uint8 [B,H,W,3] or fp32 [B,3,H,W], H and W multiples of the patch size); ``init`` is ``"sample"`` or fp32 rows [k, D].
    ``assign_clusters`` passes its centroids as ``init`` with ``k=None`` and ``iters=0``.  Every ``ValueError`` is raised here, before
    any device use."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"expected the frames as a tensor, uint8 [B,H,W,3] or fp32 [B,3,H,W], got {type(x).__name__}")
    kind, B, H, W = frame_layout(x, patch, multiple=True, one_patch=True, non_empty=True)
    hp, wp = H // patch, W // patch
    N = int(B) * hp * wp
    if k is not None:
        k = _int_in(k, 1, KMEANS_MAX_K, "k")
    iters = _int_in(iters, 0, 1 << 20, "iters")
    n_init = _int_in(n_init, 1, 1 << 20, "n_init")
    seed = _int_in(seed, -(1 << 62), 1 << 62, "seed")
    chunk = _int_in(chunk, 1, 1 << 20, "chunk")
    if isinstance(init, str):
        if init != "sample" or k is None:
            raise ValueError(f"init must be 'sample' or fp32 rows [k, {embed_dim}], got {init!r}")
        if k > N:
            raise ValueError(f"init='sample' draws k = {k} distinct points, but the frames have only N = {N} patch cells")
        how = "sample"
    else:
        k, how = _centroid_rows(init, k, embed_dim, "init" if k is not None else "centroids"), "rows"
    try:
        OH, OW = out_size(size, (H, W))
    except (TypeError, ValueError):
        raise ValueError(f"size must be a pair (OH, OW), got {size!r}") from None
    if OH < hp or OW < wp:
        raise ValueError(f"size {(OH, OW)} is smaller than the patch grid {(hp, wp)}")
    return KMeansPlan(kind, int(B), int(H), int(W), hp, wp, N, k, iters, how, seed, n_init, OH, OW, chunk)


# ---- unsupervised foreground masks: normalized cut on a 1-bit patch graph (include/dinoseg.h: dinoseg_op_ncut_graph) ----
NCUT_MAX_CELLS = 10160         # dinoseg_ncut_max_cells(): what the vectors z, xv, r, u leave of the 160 KiB of LDS (checked by tests)
NCUT_SPLIT_MAX_CELLS = 40640   # dinoseg_ncut_split_max_cells(): what the one vector xv leaves of the 160 KiB of LDS of a row workgroup
NCUT_MAX_ITERS = 4096


class NcutPlan(NamedTuple):
    """What a normalized-cut call was asked for, validated: the frames' layout, the patch grid, the rule's parameters (``tau`` as the
    fp32 value the graph launch compares against), the output size, and ``split``: 0 for the one-workgroup launch, -1 for the split
    launches with the library's choice of rows per workgroup, R >= 1 for the split launches with R rows per workgroup."""
    kind: int
    B: int
    H: int
    W: int
    hp: int
    wp: int
    tau: float
    eps: float
    iters: int
    seed: int
    OH: int
    OW: int
    chunk: int
    split: int = 0


def ncut_start(n: int, seed: int) -> torch.Tensor:
    """The start vector of the power iteration: a seeded host normal vector, fp32 [n] (the library has no device random numbers).
    Every frame of a call starts from the same vector."""
    n = int(n)
    if n < 1:
        raise ValueError(f"the start vector has n = {n} cells (positive)")
    return torch.randn(n, generator=torch.Generator().manual_seed(int(seed)), dtype=torch.float32)


def ncut_plan(patch: int, x: torch.Tensor, tau=0.2, eps=1e-5, iters=64, seed=0, size=None, chunk=32, split=False) -> NcutPlan:
    """The shape and parameter checks of ``DINOSeg.ncut`` without a device.  ``x`` is the batch (uint8 [B,H,W,3] or fp32 [B,3,H,W], H
    and W multiples of the patch size).  ``split``: ``False`` for the one-workgroup launch, ``True`` for the split launches with the
    library's choice of rows per workgroup, an int >= 1 for that many rows per workgroup.  Every ``ValueError`` is raised here, before
    any device use."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"expected the frames as a tensor, uint8 [B,H,W,3] or fp32 [B,3,H,W], got {type(x).__name__}")
    kind, B, H, W = frame_layout(x, patch, multiple=True, one_patch=True, non_empty=True)
    hp, wp = H // patch, W // patch
    for v in (tau, eps):
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"tau and eps must be numbers, got {tau!r} and {eps!r}")
    tau32, eps = float(np.float32(tau)), float(eps)                     # tau is rounded once to fp32, here
    if not (math.isfinite(tau32) and -1.0 < tau32 < 1.0):
        raise ValueError(f"tau = {tau!r} must be finite and inside (-1, 1)")
    if not 0.0 <= eps < 1.0:
        raise ValueError(f"eps = {eps!r} must be inside [0, 1)")
    iters = _int_in(iters, 0, NCUT_MAX_ITERS, "iters")
    seed = _int_in(seed, -(1 << 62), 1 << 62, "seed")
    chunk = _int_in(chunk, 1, 1 << 20, "chunk")
    if isinstance(split, (bool, np.bool_)):
        split = -1 if split else 0
    elif isinstance(split, (int, np.integer)) and split >= 1:
        split = min(int(split), NCUT_SPLIT_MAX_CELLS)                   # (rows per workgroup beyond the frame's rows: the whole frame)
    else:
        raise ValueError(f"split must be False, True or a number of rows per workgroup >= 1, got {split!r}")
    if split and hp * wp > NCUT_SPLIT_MAX_CELLS:
        raise ValueError(f"the patch grid {(hp, wp)} has {hp * wp} cells; with split, the one vector of at most {NCUT_SPLIT_MAX_CELLS} "
                         f"(NCUT_SPLIT_MAX_CELLS) fits the LDS of a row workgroup")
    if not split and hp * wp > NCUT_MAX_CELLS:
        raise ValueError(f"the patch grid {(hp, wp)} has {hp * wp} cells; the vectors of at most {NCUT_MAX_CELLS} fit the LDS of the "
                         f"one workgroup that iterates a frame")
    try:
        OH, OW = out_size(size, (H, W))
    except (TypeError, ValueError):
        raise ValueError(f"size must be a pair (OH, OW), got {size!r}") from None
    if OH < hp or OW < wp:
        raise ValueError(f"size {(OH, OW)} is smaller than the patch grid {(hp, wp)}")
    return NcutPlan(kind, int(B), int(H), int(W), hp, wp, tau32, eps, iters, seed, OH, OW, chunk, split)


# ---- connected components of a label map and their object table (include/dinoseg.h: dinoseg_op_components) ----
COMPONENTS_MAX_SIDE = 8192            # DINOSEG_COMPONENTS_MAX_SIDE
COMPONENTS_MAX_OBJECTS = 1 << 20      # DINOSEG_COMPONENTS_MAX_OBJECTS


class ComponentsPlan(NamedTuple):
    """What a connected-components call was asked for, validated: the frames' shape (``promoted``: the caller gave one [H, W] map),
    the rule's parameters (``ignore`` as the operator takes it: -1 for "negatives only") and the rows of the object table."""
    B: int
    H: int
    W: int
    connectivity: int
    ignore: int
    max_objects: int
    promoted: bool


def components_plan(labels: torch.Tensor, connectivity=4, ignore=None, max_objects=256) -> ComponentsPlan:
    """The shape and parameter checks of ``DINOSeg.components`` without a device.  ``labels``: a map [B, H, W] or [H, W] of any
    integer dtype (bool and uint8 included) whose values fit int32.  Every ``ValueError`` is raised here, before any device use."""
    if not isinstance(labels, torch.Tensor):
        raise ValueError(f"expected the label map as a tensor, integer [B,H,W] or [H,W], got {type(labels).__name__}")
    if labels.is_floating_point() or labels.is_complex():
        raise ValueError(f"the label map must have an integer dtype (bool and uint8 included), got {labels.dtype}")
    if labels.dim() not in (2, 3):
        raise ValueError(f"the label map must be [B,H,W] or [H,W], got {tuple(labels.shape)}")
    promoted = labels.dim() == 2
    B, H, W = (1, *labels.shape) if promoted else labels.shape
    B, H, W = int(B), int(H), int(W)
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"the label map {tuple(labels.shape)} is empty")
    if H > COMPONENTS_MAX_SIDE or W > COMPONENTS_MAX_SIDE:
        raise ValueError(f"frames of {H} x {W} exceed {COMPONENTS_MAX_SIDE} (COMPONENTS_MAX_SIDE) along a side")
    if B * H * W >= 1 << 31:
        raise ValueError(f"{B} frames of {H} x {W} hold {B * H * W} pixels; linear indices must stay below 2^31")
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    ignore = -1 if ignore is None else _int_in(ignore, -(1 << 31), (1 << 31) - 1, "ignore")
    max_objects = _int_in(max_objects, 1, COMPONENTS_MAX_OBJECTS, "max_objects")
    return ComponentsPlan(B, H, W, int(connectivity), ignore, max_objects, promoted)


# ---- multi-object discovery: recursive normalized cuts (include/dinoseg.h: dinoseg_op_maskcut) ----
MASKCUT_MAX_OBJECTS = 16              # DINOSEG_MASKCUT_MAX_OBJECTS


class MaskCutPlan(NamedTuple):
    """What a multi-object discovery call was asked for, validated: the plan of every round's cut (split launches only), the
    number of rounds and the connectivity of the component around the seed."""
    ncut: NcutPlan
    max_objects: int
    connectivity: int


def maskcut_plan(patch: int, x: torch.Tensor, max_objects=3, tau=0.2, eps=1e-5, iters=64, seed=0, size=None, chunk=32, split=True,
                 connectivity=4) -> MaskCutPlan:
    """The shape and parameter checks of ``DINOSeg.discover_all`` without a device: those of ``ncut_plan`` with ``split``, then
    ``max_objects`` in 1 .. ``MASKCUT_MAX_OBJECTS``, ``connectivity`` 4 or 8, and ``split=False`` refused (the rounds run on the split
    launches only).  Every ``ValueError`` is raised here, before any device use."""
    if isinstance(split, (bool, np.bool_)) and not split:
        raise ValueError("discover_all runs on the split launches only: split must be True or a number of rows per workgroup >= 1")
    plan = ncut_plan(patch, x, tau, eps, iters, seed, size, chunk, split)
    max_objects = _int_in(max_objects, 1, MASKCUT_MAX_OBJECTS, "max_objects")
    if isinstance(connectivity, bool) or not isinstance(connectivity, (int, np.integer)) or int(connectivity) not in (4, 8):
        raise ValueError(f"connectivity must be 4 or 8, got {connectivity!r}")
    if plan.hp > COMPONENTS_MAX_SIDE or plan.wp > COMPONENTS_MAX_SIDE:
        raise ValueError(f"the patch grid {(plan.hp, plan.wp)} exceeds {COMPONENTS_MAX_SIDE} (COMPONENTS_MAX_SIDE) along a side")
    return MaskCutPlan(plan, max_objects, int(connectivity))


# ---- PCA of patch features (include/dinoseg.h: dinoseg_op_token_moments, dinoseg_op_pca_project, dinoseg_op_pca_colour) ----
PCA_MAX_Q = 256                # include/dinoseg.h: DINOSEG_PCA_MAX_Q, the components dinoseg_op_pca_project takes
PCA_MAX_SIDE = 16384           # an output side of dinoseg_op_pca_colour


class PcaPlan(NamedTuple):
    """What a PCA call (``PCAFitter.update``, ``pca_fit``, ``pca_project``, ``pca_map``, a projected ``MemoryBank``) was asked for,
    validated: the frames' layout, the patch grid, the components, whether a ``keep`` mask came, the blocks the features are taken
    after, the chunk, the output size and the colour range (``None``: the call's own minimum / maximum)."""
    kind: int
    B: int
    H: int
    W: int
    hp: int
    wp: int
    q: int
    keep: bool
    n_blocks: int
    chunk: int
    OH: int
    OW: int
    lo: Optional[Tuple[float, float, float]]
    hi: Optional[Tuple[float, float, float]]


def _colour_range(v, what: str) -> Optional[Tuple[float, float, float]]:
    if v is None:
        return None
    try:
        if isinstance(v, (torch.Tensor, np.ndarray)):
            v = v.tolist()
        vals = [float(v)] * 3 if isinstance(v, (int, float)) else [float(t) for t in v]
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a number or three numbers, got {v!r}") from None
    if len(vals) != 3 or not all(math.isfinite(t) for t in vals):
        raise ValueError(f"{what} must be a finite number or three of them, got {v!r}")
    return (vals[0], vals[1], vals[2])


def pca_projection(pca, embed_dim: int, what: str = "pca", bank: bool = False, blocks=None):
    """The checks of a fitted projection handed to a call: a ``FeaturePCA`` of the model's width with at most ``PCA_MAX_Q``
    components; for a memory bank (``bank``) a number of components that is a multiple of 64, the width the similarity operators
    take; ``blocks``, when given, must be the projection's ``n_blocks``."""
    from .pca import FeaturePCA
    if not isinstance(pca, FeaturePCA):
        raise ValueError(f"{what} must be a FeaturePCA, got {type(pca).__name__}")
    if pca.dim != int(embed_dim):
        raise ValueError(f"{what} was fitted on features of width {pca.dim}, the model's embed_dim is {embed_dim}")
    if not 1 <= pca.q <= PCA_MAX_Q:
        raise ValueError(f"{what} has {pca.q} components, the projection takes 1..{PCA_MAX_Q}")
    if bank and pca.q % 64 != 0:
        raise ValueError(f"a memory bank's projection needs a number of components that is a multiple of 64, got q = {pca.q}")
    if blocks is not None and int(blocks) != pca.n_blocks:
        raise ValueError(f"{what} was fitted with n_blocks = {pca.n_blocks}, the call asks for n_blocks = {blocks}")
    return pca


def pca_plan(patch: int, embed_dim: int, max_blocks: int, x: torch.Tensor, q=None, keep=None, n_blocks=0, chunk=32, pca=None,
             size=None, lo=None, hi=None, colour: bool = False) -> PcaPlan:
    """The shape and parameter checks of the PCA calls without a device.  ``x`` is the batch (uint8 [B,H,W,3] or fp32 [B,3,H,W], H
    and W multiples of the patch size).  Fitting: ``q`` components (1 .. min(``PCA_MAX_Q``, ``embed_dim``); ``None`` for an
    ``update``, which takes none), ``keep`` a bool / uint8 [B, n] mask, ``n_blocks`` in 0 .. ``max_blocks``.  Projecting: ``pca`` a
    ``FeaturePCA`` of the model's width, ``n_blocks`` ``None`` or the projection's.  ``colour``: at least three components, ``size``
    at least the patch grid with sides up to ``PCA_MAX_SIDE``, ``lo`` / ``hi`` ``None`` or finite numbers.  Every ``ValueError`` is
    raised here, before any device use."""
    if not isinstance(x, torch.Tensor):
        raise ValueError(f"expected the frames as a tensor, uint8 [B,H,W,3] or fp32 [B,3,H,W], got {type(x).__name__}")
    kind, B, H, W = frame_layout(x, patch, multiple=True, one_patch=True, non_empty=True)
    hp, wp = H // patch, W // patch
    n = hp * wp
    chunk = _int_in(chunk, 1, 1 << 20, "chunk")
    if pca is not None:
        pca_projection(pca, embed_dim, blocks=n_blocks)
        n_blocks, q = pca.n_blocks, pca.q
    else:
        n_blocks = _int_in(n_blocks, 0, int(max_blocks), "n_blocks")
        if q is not None:
            q = _int_in(q, 1, min(PCA_MAX_Q, int(embed_dim)), "q")
    if keep is not None:
        if not isinstance(keep, torch.Tensor) or keep.dtype not in (torch.bool, torch.uint8) or tuple(keep.shape) != (B, n):
            raise ValueError(f"keep must be a bool or uint8 mask [B = {B}, n = {n}], got "
                             f"{getattr(keep, 'dtype', type(keep).__name__)} {tuple(getattr(keep, 'shape', ()))}")
    try:
        OH, OW = out_size(size, (H, W))
    except (TypeError, ValueError):
        raise ValueError(f"size must be a pair (OH, OW), got {size!r}") from None
    if colour:
        if q is None or q < 3:
            raise ValueError(f"a colour map needs at least 3 components, the projection has {q}")
        if OH < hp or OW < wp:
            raise ValueError(f"size {(OH, OW)} is smaller than the patch grid {(hp, wp)}")
        if OH > PCA_MAX_SIDE or OW > PCA_MAX_SIDE:
            raise ValueError(f"size {(OH, OW)} exceeds {PCA_MAX_SIDE} along a side")
    lo, hi = _colour_range(lo, "lo"), _colour_range(hi, "hi")
    return PcaPlan(kind, int(B), int(H), int(W), hp, wp, 0 if q is None else int(q), keep is not None, int(n_blocks), chunk, OH, OW,
                   lo, hi)
