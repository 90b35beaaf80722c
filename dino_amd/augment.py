"""Augmentation of fine-tuning frames and label masks on the device: the reference's ``get_augmented_transforms()``
(pl_torch_modules.py:44-57 -- RandomResizedCrop, ShiftScaleRotate, HorizontalFlip, ColorJitter(brightness=0.5),
GaussianBlur(blur_limit=(3, 41)), Normalize, the mask nearest-resized to the patch grid) as one or two HIP launches
(``csrc/augment.hip``, C-ABI ``dinoseg_op_augment``).

The device code is a pure function of a per-frame parameter table (``dinoseg_augment_frame`` in ``include/dinoseg.h``, 36 32-bit
words; here an int32 ``[B, 36]`` tensor with the floats bit-cast): no device random numbers, Q16 integer coordinates, no atomics.
``augment_table`` fills the table from explicit parameters, ``draw_reference_augment`` from the reference recipe's random draws
(a seeded ``torch.Generator`` on the host), ``Augmenter`` is the hook ``DINOSeg.fit(augment=...)`` takes.

Deviations from albumentations, by design: the crop-resize, the shift-scale-rotate and the flip are composed into ONE inverse
affine, so the frame is interpolated once instead of three times; there is no uint8 rounding between the stages (one rounding at
the end, none for the normalised fp32 output); ``ColorJitter``'s implicit default contrast / saturation / hue ranges are not drawn
(``sat`` is exposed in the table but stays 1 in the reference recipe; hue and contrast about the frame mean are out of scope).
"""
from __future__ import annotations

import math
from typing import Callable, Optional, Tuple

import numpy as np
import torch

WORDS = 36                      # 32-bit words of one dinoseg_augment_frame
MAX_RADIUS = 20                 # kernel size 41
MAX_SIDE = 16384
# word offsets of the fields
_A, _BORDER, _VOID, _FILL, _GAIN, _BIAS, _SAT, _RADIUS, _W = 0, 6, 7, 8, 11, 12, 13, 14, 15
_BORDERS = {"reflect": 0, "constant": 1}


def _size(v, what: str) -> Tuple[int, int]:
    try:
        h, w = (int(v[0]), int(v[1])) if len(v) == 2 else (None, None)
    except TypeError:
        h = w = None
    if h is None or h < 1 or w < 1 or h > MAX_SIDE or w > MAX_SIDE:
        raise ValueError(f"{what} must be (rows, cols) with 1 <= side <= {MAX_SIDE}, got {v!r}")
    return h, w


def _per_frame(v, B: int, width: int, what: str) -> np.ndarray:
    """A scalar (width 0) / a width-tuple, or B of them -> fp64 [B] / [B, width]; finite."""
    a = np.asarray(v, dtype=np.float64)
    shape = (B,) if width == 0 else (B, width)
    if a.shape == shape[1:] or a.shape == shape:
        a = np.broadcast_to(a, shape)
    else:
        raise ValueError(f"{what}: expected {'a scalar' if width == 0 else f'{width} values'} or one per frame ({B}), "
                         f"got shape {a.shape}")
    if not np.isfinite(a).all():
        raise ValueError(f"{what} must be finite")
    return a


def gaussian_taps(ksize: int) -> np.ndarray:
    """fp64 taps w[0 .. r] of an odd kernel size (3..41): OpenCV's rule for sigma = 0, ``sigma = 0.3 ((ksize - 1) / 2 - 1) + 0.8``
    (what albumentations' GaussianBlur passes), ``exp(-k^2 / (2 sigma^2))`` normalised over the whole kernel."""
    r = (ksize - 1) // 2
    sigma = 0.3 * ((ksize - 1) * 0.5 - 1.0) + 0.8
    k = np.arange(r + 1, dtype=np.float64)
    w = np.exp(-(k * k) / (2.0 * sigma * sigma))
    return w / (w[0] + 2.0 * w[1:].sum())


def augment_table(B: int, src, out, *, crop=None, angle=0, scale=1, shift=(0, 0), flip=False, border="reflect", fill=(124, 116, 104),
                  void_label=255, gain=1, bias=0, sat=1, ksize=0) -> torch.Tensor:
    """The parameter table of ``B`` frames, CPU int32 ``[B, 36]``.  Every argument after ``out`` is one value for all frames or a
    sequence with one value per frame.

    Geometry, in this order: the crop box ``(top, left, h, w)`` of the ``src = (H, W)`` frame (default: the whole frame) is resized
    to ``out = (OH, OW)`` by the pixel-centre-aligned linear map (output pixel centre ``ox + 1/2`` -> ``left + (ox + 1/2) w / OW``:
    ``F.interpolate(align_corners=False)``'s coordinates); the result is rotated by ``angle`` degrees (positive = counter-clockwise,
    ``cv2.getRotationMatrix2D``) and scaled by ``scale`` about the output centre and shifted by ``shift = (dx, dy)`` fractions of
    the output width / height; then mirrored left-right where ``flip``.  All of it is composed in fp64 into ONE inverse affine
    (output pixel -> source) and rounded to Q16; the translation words hold the output half-pixel term.
    ``border``: "reflect" (reflect-101) or "constant" (``fill`` RGB per tap, ``void_label`` for the mask).  Colour:
    ``v = gain v + bias``, then ``v = gray + sat (v - gray)``, clamped to [0, 255].  ``ksize``: 0 (no blur) or an odd Gaussian kernel
    size 3..41 (``gaussian_taps``); the output sides must exceed its radius.  Bad values raise ``ValueError``."""
    B = int(B)
    if B < 1:
        raise ValueError(f"B must be positive, got {B}")
    H, W = _size(src, "src")
    OH, OW = _size(out, "out")
    crop = _per_frame((0, 0, H, W) if crop is None else crop, B, 4, "crop (top, left, h, w)")
    if (crop[:, 2:] <= 0).any():
        raise ValueError("crop: h and w must be positive")
    angle = _per_frame(angle, B, 0, "angle")
    scale = _per_frame(scale, B, 0, "scale")
    if (scale <= 0).any():
        raise ValueError("scale must be positive")
    shift = _per_frame(shift, B, 2, "shift (dx, dy)")
    fill = _per_frame(fill, B, 3, "fill (r, g, b)")
    gain, bias, sat = (_per_frame(v, B, 0, n) for v, n in ((gain, "gain"), (bias, "bias"), (sat, "sat")))
    flip = np.broadcast_to(np.asarray(flip, dtype=bool), (B,)) if np.ndim(flip) == 0 else np.asarray(flip, dtype=bool)
    if flip.shape != (B,):
        raise ValueError(f"flip: expected a bool or one per frame ({B}), got shape {flip.shape}")
    borders = [border] * B if isinstance(border, str) else list(border)
    if len(borders) != B or any(b not in _BORDERS for b in borders):
        raise ValueError(f"border must be 'reflect' or 'constant' (one, or one per frame), got {border!r}")
    void = _per_frame(void_label, B, 0, "void_label")
    if (void != np.floor(void)).any() or (np.abs(void) >= 2 ** 31).any():
        raise ValueError("void_label must be a 32-bit integer")
    ks = _per_frame(ksize, B, 0, "ksize")
    for k in ks:
        if not (k == 0 or (k == int(k) and int(k) % 2 == 1 and 3 <= k <= 2 * MAX_RADIUS + 1)):
            raise ValueError(f"ksize must be 0 or odd in 3..{2 * MAX_RADIUS + 1}, got {k:g}")
        if (int(k) - 1) // 2 >= min(OH, OW) and k:
            raise ValueError(f"ksize {int(k)} has radius {(int(k) - 1) // 2}: the output sides ({OH} x {OW}) must exceed it")

    table = np.zeros((B, WORDS), dtype=np.int32)
    fl = table.view(np.float32)
    cx, cy = OW * 0.5, OH * 0.5
    for b in range(B):
        top, left, h, w = crop[b]
        th = math.radians(angle[b])
        ci, si = math.cos(th) / scale[b], math.sin(th) / scale[b]
        px, py = cx + shift[b, 0] * OW, cy + shift[b, 1] * OH
        crop_inv = np.array([[w / OW, 0.0, left], [0.0, h / OH, top], [0.0, 0.0, 1.0]])
        # the inverse of [[al, be], [-be, al]] (q - c) + c + shift, al = scale cos, be = scale sin
        ssr_inv = np.array([[ci, -si, cx - ci * px + si * py], [si, ci, cy - si * px - ci * py], [0.0, 0.0, 1.0]])
        flip_inv = np.array([[-1.0, 0.0, float(OW)], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) if flip[b] else np.eye(3)
        m = crop_inv @ ssr_inv @ flip_inv
        q = np.array([m[0, 0], m[0, 1], m[0, 2] + 0.5 * (m[0, 0] + m[0, 1]), m[1, 0], m[1, 1], m[1, 2] + 0.5 * (m[1, 0] + m[1, 1])])
        q = np.rint(q * 65536.0)
        if (np.abs(q) >= 2.0 ** 31).any():
            raise ValueError(f"frame {b}: the inverse affine {m[:2].tolist()} does not fit Q16 in 32 bits")
        table[b, _A:_A + 6] = q.astype(np.int64)
        table[b, _BORDER] = _BORDERS[borders[b]]
        table[b, _VOID] = int(void[b])
        fl[b, _FILL:_FILL + 3] = fill[b]
        fl[b, _GAIN], fl[b, _BIAS], fl[b, _SAT] = gain[b], bias[b], sat[b]
        k = int(ks[b])
        if k:
            r = (k - 1) // 2
            table[b, _RADIUS] = r
            fl[b, _W:_W + r + 1] = gaussian_taps(k)
    return torch.from_numpy(table)


def unpack_table(table: torch.Tensor) -> dict:
    """The fields of an int32 [B, 36] table as numpy arrays: a int64 [B, 6], border, void_label, radius int64 [B], fill fp32 [B, 3],
    gain, bias, sat fp32 [B], w fp32 [B, 21]."""
    t = table.detach().cpu().contiguous().numpy()
    f = t.view(np.float32)
    return {"a": t[:, _A:_A + 6].astype(np.int64), "border": t[:, _BORDER].astype(np.int64), "void_label": t[:, _VOID].astype(np.int64),
            "fill": f[:, _FILL:_FILL + 3].copy(), "gain": f[:, _GAIN].copy(), "bias": f[:, _BIAS].copy(), "sat": f[:, _SAT].copy(),
            "radius": t[:, _RADIUS].astype(np.int64), "w": f[:, _W:_W + MAX_RADIUS + 1].copy()}


def validate_table(table, B: int, OH: int, OW: int) -> int:
    """The host-side check of a table before it is uploaded: int32 [B, 36], borders 0 / 1, radii 0..20 and below both output
    sides, finite colour parameters, fills and taps.  Returns the largest radius.  (A device tensor is read back for the check.)"""
    if not isinstance(table, torch.Tensor) or table.dtype != torch.int32 or table.dim() != 2 or table.shape[1] != WORDS:
        got = (table.dtype, tuple(table.shape)) if isinstance(table, torch.Tensor) else type(table).__name__
        raise ValueError(f"the augmentation table must be an int32 [B, {WORDS}] tensor, got {got}")
    if table.shape[0] != B:
        raise ValueError(f"the augmentation table has {table.shape[0]} rows for {B} frames")
    f = unpack_table(table)
    if ((f["border"] != 0) & (f["border"] != 1)).any():
        raise ValueError("augmentation table: border must be 0 (reflect-101) or 1 (constant)")
    if (f["radius"] < 0).any() or (f["radius"] > MAX_RADIUS).any():
        raise ValueError(f"augmentation table: radius outside 0..{MAX_RADIUS}")
    rmax = int(f["radius"].max())
    if rmax >= min(OH, OW):
        raise ValueError(f"augmentation table: radius {rmax} needs output sides above it, got {OH} x {OW}")
    used = np.arange(MAX_RADIUS + 1)[None, :] <= f["radius"][:, None]
    ok = all(np.isfinite(f[k]).all() for k in ("fill", "gain", "bias", "sat")) and np.isfinite(np.where(used, f["w"], 0.0)).all()
    if not ok:
        raise ValueError("augmentation table: non-finite colour parameter, fill or tap")
    return rmax


def draw_reference_parameters(B: int, src, out, generator: torch.Generator) -> dict:
    """The reference recipe's random draws (pl_torch_modules.py:48-52) for ``B`` frames as keyword arguments of ``augment_table``
    (numpy arrays with one entry per frame), from ``generator`` alone -- a fixed number of uniform draws per frame, so the same
    seed gives the same parameters:

    * resized crop, p = .75: area fraction U(.25, 1) of the frame, log aspect ratio U(log .9, log 1.1), ``w = round(sqrt(area
      ratio))``, ``h = round(sqrt(area / ratio))``; up to 10 attempts to fit the frame, then the whole frame; position uniform;
    * shift-scale-rotate, p = .25: shifts U(-.4, .4), scale U(.9, 1.1), angle U(-15, 15) degrees, reflect-101 border;
    * horizontal flip, p = .5;  brightness, p = .5: gain U(.5, 1.5);  Gaussian blur, p = .25: odd ksize uniform in 3..41."""
    B = int(B)
    if B < 1:
        raise ValueError(f"B must be positive, got {B}")
    H, W = _size(src, "src")
    _size(out, "out")
    u = torch.rand((B, 51), dtype=torch.float64, generator=generator).numpy()
    crop = np.tile(np.array([0.0, 0.0, H, W]), (B, 1))
    for b in range(B):
        if u[b, 0] >= 0.75:
            continue
        for k in range(10):
            ua, ur, uy, ux = u[b, 1 + 4 * k:5 + 4 * k]
            area = H * W * (0.25 + 0.75 * ua)
            ratio = math.exp(math.log(0.9) + (math.log(1.1) - math.log(0.9)) * ur)
            w, h = int(round(math.sqrt(area * ratio))), int(round(math.sqrt(area / ratio)))
            if 0 < w <= W and 0 < h <= H:
                crop[b] = (min(int(uy * (H - h + 1)), H - h), min(int(ux * (W - w + 1)), W - w), h, w)
                break
    ssr = u[:, 41] < 0.25
    shift = np.where(ssr[:, None], -0.4 + 0.8 * u[:, 42:44], 0.0)
    scale = np.where(ssr, 0.9 + 0.2 * u[:, 44], 1.0)
    angle = np.where(ssr, -15.0 + 30.0 * u[:, 45], 0.0)
    flip = u[:, 46] < 0.5
    gain = np.where(u[:, 47] < 0.5, 0.5 + u[:, 48], 1.0)
    ksize = np.where(u[:, 49] < 0.25, 3 + 2 * np.minimum((u[:, 50] * 20).astype(np.int64), 19), 0)
    return dict(crop=crop, angle=angle, scale=scale, shift=shift, flip=flip, border="reflect", gain=gain, ksize=ksize)


def draw_reference_augment(B: int, src, out, generator: torch.Generator) -> torch.Tensor:
    """The table (CPU int32 ``[B, 36]``) of the reference recipe's draws: ``augment_table`` of ``draw_reference_parameters``."""
    return augment_table(B, src, out, **draw_reference_parameters(B, src, out, generator))


class Augmenter:
    """The hook of ``DINOSeg.fit(augment=...)``: ``augmenter(model, x, y) -> (x_aug, y_aug)`` draws a table for the batch from its
    own seeded generator (two Augmenters with the same seed give the same sequence) and runs ``model.augment``.  ``x`` uint8
    [B,H,W,3], ``y`` an integer [B,H,W] mask; ``labels``: "patch" (int64 [B, (OH/p)(OW/p)], the reference's mask at the patch
    grid, for ``fused_training_step``) or "pixel" (int64 [B,OH,OW], for ``fused_training_step_dense``); ``out_kind``: "f32"
    (normalised [B,3,OH,OW]) or "u8" ([B,OH,OW,3]); ``draw(B, src, out, generator)`` returns the table."""

    def __init__(self, out=(480, 480), seed: int = 0, labels: str = "patch", out_kind: str = "f32",
                 draw: Callable = draw_reference_augment):
        self.out = _size(out, "out")
        if labels not in ("patch", "pixel"):
            raise ValueError(f"labels must be 'patch' or 'pixel', got {labels!r}")
        if out_kind not in ("f32", "u8"):
            raise ValueError(f"out_kind must be 'f32' or 'u8', got {out_kind!r}")
        self.labels, self.out_kind, self.draw = labels, out_kind, draw
        self.generator = torch.Generator().manual_seed(int(seed))

    def __call__(self, model, x: torch.Tensor, y: Optional[torch.Tensor]):
        if x.dim() != 4:
            raise ValueError(f"expected uint8 [B,H,W,3], got {tuple(x.shape)}")
        table = self.draw(int(x.shape[0]), (int(x.shape[1]), int(x.shape[2])), self.out, self.generator)
        return model.augment(x, y, table, out=self.out, out_kind=self.out_kind, labels=self.labels)


__all__ = ["Augmenter", "augment_table", "draw_reference_augment", "draw_reference_parameters", "gaussian_taps", "unpack_table", "validate_table", "WORDS", "MAX_RADIUS"]
