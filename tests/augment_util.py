"""Shared by tests/test_augment_cpu.py and tests/test_augment_gpu.py: the stated rule of dinoseg_op_augment (include/dinoseg.h)
restated in int64 / fp64 numpy, and torch's own fp64 routes on the CPU as independent yardsticks of that restatement."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

from dino_amd.augment import unpack_table

MEAN = np.array((0.485, 0.456, 0.406))
STD = np.array((0.229, 0.224, 0.225))


def fold101(i, n):
    """reflect-101 of int64 indices onto [0, n): period 2 (n - 1); a side of 1 folds to 0."""
    i = np.asarray(i, dtype=np.int64)
    if n == 1:
        return np.zeros_like(i)
    P = 2 * (n - 1)
    m = np.mod(i, P)
    return np.where(m < n, m, P - m)


def source_coords(a, OH, OW):
    """(Ux, Uy) int64 [OH, OW]: the Q16 source coordinate of every output pixel."""
    ox = np.arange(OW, dtype=np.int64)[None, :]
    oy = np.arange(OH, dtype=np.int64)[:, None]
    a = [int(v) for v in a]
    return a[0] * ox + a[1] * oy + a[2], a[3] * ox + a[4] * oy + a[5]


def warp_frame(frame, a, border, fill, OH, OW):
    """The image rule before colour: frame [H, W, 3] (any real dtype) -> fp64 [OH, OW, 3]."""
    H, W = frame.shape[:2]
    src = frame.astype(np.float64)
    Ux, Uy = source_coords(a, OH, OW)
    Vx, Vy = Ux - 32768, Uy - 32768
    x0, y0 = Vx >> 16, Vy >> 16
    lx, ly = (Vx & 0xFFFF) / 65536.0, (Vy & 0xFFFF) / 65536.0

    def tap(yy, xx):
        v = src[fold101(yy, H), fold101(xx, W)]
        if border & 1:
            inside = (yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)
            v = np.where(inside[..., None], v, np.asarray(fill, dtype=np.float64)[None, None, :])
        return v

    v00, v01, v10, v11 = tap(y0, x0), tap(y0, x0 + 1), tap(y0 + 1, x0), tap(y0 + 1, x0 + 1)
    top = v00 + (v01 - v00) * lx[..., None]
    bot = v10 + (v11 - v10) * lx[..., None]
    return top + (bot - top) * ly[..., None]


def warp_mask(mask, a, border, void_label, OH, OW):
    """The label rule: mask [H, W] -> int64 [OH, OW]."""
    H, W = mask.shape
    Ux, Uy = source_coords(a, OH, OW)
    sx, sy = Ux >> 16, Uy >> 16
    lab = mask.astype(np.int64)[fold101(sy, H), fold101(sx, W)]
    if border & 1:
        inside = (sy >= 0) & (sy < H) & (sx >= 0) & (sx < W)
        lab = np.where(inside, lab, np.int64(void_label))
    return lab


def colour(v, gain, bias, sat):
    v = float(gain) * v + float(bias)
    g = 0.299 * v[..., 0] + 0.587 * v[..., 1] + 0.114 * v[..., 2]
    v = g[..., None] + float(sat) * (v - g[..., None])
    return np.clip(v, 0.0, 255.0)


def blur(v, r, w):
    """Separable, horizontal then vertical, output coordinates folded by reflect-101: v fp64 [OH, OW, 3]; w the taps w[0 .. r]."""
    if r == 0:
        return v
    OH, OW = v.shape[:2]
    w = np.asarray(w, dtype=np.float64)
    h = np.zeros_like(v)
    for d in range(-r, r + 1):
        h += w[abs(d)] * v[:, fold101(np.arange(OW) + d, OW)]
    out = np.zeros_like(v)
    for d in range(-r, r + 1):
        out += w[abs(d)] * h[fold101(np.arange(OH) + d, OH)]
    return out


def restate(frames, masks, table, OH, OW, patch=None, max_radius=20):
    """The whole rule on numpy inputs (frames uint8 [B,H,W,3], masks integer [B,H,W] or None, table int32 [B,36] tensor) ->
    dict: value fp64 [B,OH,OW,3] on the 0..255 scale (before the output conversion), norm fp64 [B,3,OH,OW], labels int64
    [B,OH,OW] (or None), patch_labels int64 [B,(OH/p)(OW/p)] (with patch)."""
    f = unpack_table(table)
    B = frames.shape[0]
    value = np.zeros((B, OH, OW, 3))
    labels = None if masks is None else np.zeros((B, OH, OW), dtype=np.int64)
    for b in range(B):
        v = warp_frame(frames[b], f["a"][b], int(f["border"][b]), f["fill"][b], OH, OW)
        v = colour(v, f["gain"][b], f["bias"][b], f["sat"][b])
        r = min(max(int(f["radius"][b]), 0), max_radius)
        value[b] = blur(v, r, f["w"][b])
        if masks is not None:
            labels[b] = warp_mask(masks[b], f["a"][b], int(f["border"][b]), int(f["void_label"][b]), OH, OW)
    out = {"value": value, "norm": ((value / 255.0 - MEAN) / STD).transpose(0, 3, 1, 2), "labels": labels, "patch_labels": None}
    if patch and labels is not None:
        out["patch_labels"] = labels[:, ::patch, ::patch].reshape(B, -1)
    return out


def value_bar(table, max_radius=20):
    """Per frame, on the 0..255 scale: (16 + 2 (2r + 1)) 2^-24 max(256, 255 |gain| + |bias|) -- 3 lerps, at most 6 colour roundings,
    one rounding per tap and pass, and slack, each of at most half a unit in the last place of the largest magnitude in play."""
    f = unpack_table(table)
    r = np.clip(f["radius"], 0, max_radius).astype(np.float64)
    mag = np.maximum(256.0, 255.0 * np.abs(f["gain"].astype(np.float64)) + np.abs(f["bias"].astype(np.float64)))
    return (16.0 + 2.0 * (2.0 * r + 1.0)) * 2.0 ** -24 * mag


# ------------------------------------------------------------------------------------------------ torch yardsticks (fp64, CPU)
def torch_warp_zeros(frame, a, OH, OW):
    """border = 1 with fill = 0: the Q16 coordinates divided by 65536 in fp64 and handed to F.grid_sample(bilinear, zeros,
    align_corners=False), whose normalised coordinate g maps to the edge-convention coordinate (g + 1) side / 2."""
    H, W = frame.shape[:2]
    Ux, Uy = source_coords(a, OH, OW)
    gx = torch.from_numpy(Ux / 65536.0) * 2.0 / W - 1.0
    gy = torch.from_numpy(Uy / 65536.0) * 2.0 / H - 1.0
    grid = torch.stack([gx, gy], dim=-1)[None]
    src = torch.from_numpy(frame.astype(np.float64)).permute(2, 0, 1)[None]
    out = F.grid_sample(src, grid, mode="bilinear", padding_mode="zeros", align_corners=False)
    return out[0].permute(1, 2, 0).numpy()


def torch_warp_reflect101(frame, a, OH, OW, pad):
    """border = 0 wherever all taps stay within `pad` pixels of the frame: the frame padded by F.pad(mode="reflect") (torch's
    reflect is reflect-101) and sampled at the coordinates shifted by the pad."""
    H, W = frame.shape[:2]
    src = torch.from_numpy(frame.astype(np.float64)).permute(2, 0, 1)[None]
    src = F.pad(src, (pad, pad, pad, pad), mode="reflect")
    Ux, Uy = source_coords(a, OH, OW)
    gx = (torch.from_numpy(Ux / 65536.0) + pad) * 2.0 / (W + 2 * pad) - 1.0
    gy = (torch.from_numpy(Uy / 65536.0) + pad) * 2.0 / (H + 2 * pad) - 1.0
    out = F.grid_sample(src, torch.stack([gx, gy], dim=-1)[None], mode="bilinear", padding_mode="zeros", align_corners=False)
    return out[0].permute(1, 2, 0).numpy()


def torch_blur(v, r, w):
    """F.pad(mode="reflect") + grouped F.conv2d in fp64, horizontal then vertical: v fp64 [OH, OW, 3]."""
    x = torch.from_numpy(v).permute(2, 0, 1)[None]
    k = torch.tensor([float(w[abs(d)]) for d in range(-r, r + 1)], dtype=torch.float64)
    x = F.conv2d(F.pad(x, (r, r, 0, 0), mode="reflect"), k.view(1, 1, 1, -1).repeat(3, 1, 1, 1), groups=3)
    x = F.conv2d(F.pad(x, (0, 0, r, r), mode="reflect"), k.view(1, 1, -1, 1).repeat(3, 1, 1, 1), groups=3)
    return x[0].permute(1, 2, 0).numpy()


def torch_nearest_zeros(mask, a, OH, OW):
    """(labels by F.grid_sample(nearest, zeros), where they are comparable): torch rounds the pixel coordinate half to even where
    the rule floors, so pixels whose U lies exactly on a pixel edge are excluded."""
    H, W = mask.shape
    Ux, Uy = source_coords(a, OH, OW)
    gx = torch.from_numpy(Ux / 65536.0) * 2.0 / W - 1.0
    gy = torch.from_numpy(Uy / 65536.0) * 2.0 / H - 1.0
    src = torch.from_numpy(mask.astype(np.float64))[None, None]
    out = F.grid_sample(src, torch.stack([gx, gy], dim=-1)[None], mode="nearest", padding_mode="zeros", align_corners=False)
    off_edge = ((Ux & 0xFFFF) != 0) & ((Uy & 0xFFFF) != 0)
    return out[0, 0].numpy().astype(np.int64), off_edge


# ------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=8)
def random_batch(B, H, W, n_labels=7, seed=0):
    """(frames uint8 [B,H,W,3], masks uint8 [B,H,W] in [0, n_labels)) as numpy arrays, shared by the tests and never modified."""
    g = np.random.default_rng(1000 * H + W + seed)
    frames = g.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    masks = g.integers(0, n_labels, (B, H, W), dtype=np.uint8)
    return frames, masks
