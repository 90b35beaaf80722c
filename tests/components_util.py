"""Host restatement of the connected-components rule (include/dinoseg.h: dinoseg_op_components) and of DINOSeg.discover's composition,
numpy only.  Everything is an integer: the device must agree exactly.

The restatement works on pixels, not tiles: the list of joined pairs (rule 2) is closed transitively by hooking the larger root under
the smaller and halving paths until nothing changes (rule 3); a component's root is then its smallest linear index, its first pixel
(rule 4); the sorted first pixels give the numbers (rule 5)."""
from __future__ import annotations

from collections import deque

import numpy as np

FIELDS = ("ids", "count", "first", "label", "area", "box")


def void_of(labels, ignore):
    return (labels < 0) | (labels == ignore)


def _pairs(lab, void, connectivity):
    """the joined pairs of one frame as two arrays of linear indices"""
    H, W = lab.shape
    idx = np.arange(H * W, dtype=np.int64).reshape(H, W)
    steps = [(0, 1), (1, 0)] + ([(1, 1), (1, -1)] if connectivity == 8 else [])
    a, b = [], []
    for dy, dx in steps:
        ys = slice(0, H - dy)
        yd = slice(dy, H)
        xs, xd = (slice(0, W - dx), slice(dx, W)) if dx >= 0 else (slice(-dx, W), slice(0, W + dx))
        same = (lab[ys, xs] == lab[yd, xd]) & ~void[ys, xs] & ~void[yd, xd]
        a.append(idx[ys, xs][same])
        b.append(idx[yd, xd][same])
    return np.concatenate(a), np.concatenate(b)


def _roots(n, a, b):
    parent = np.arange(n, dtype=np.int64)
    while True:
        ra, rb = parent[a], parent[b]
        differ = ra != rb
        if not differ.any():
            return parent
        hi, lo = np.maximum(ra, rb)[differ], np.minimum(ra, rb)[differ]
        np.minimum.at(parent, hi, lo)
        while True:
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp


def components_frame(lab, connectivity, ignore, M):
    lab = np.asarray(lab).astype(np.int64)
    H, W = lab.shape
    void = void_of(lab, ignore)
    root = _roots(H * W, *_pairs(lab, void, connectivity))
    live = ~void.reshape(-1)
    firsts = np.unique(root[live])                                      # ascending: the numbering rule
    ids = np.full(H * W, -1, dtype=np.int32)
    ids[live] = np.searchsorted(firsts, root[live]).astype(np.int32)
    count = int(firsts.size)
    first = np.full(M, -1, dtype=np.int32)
    label = np.full(M, -1, dtype=np.int32)
    area = np.zeros(M, dtype=np.int32)
    box = np.zeros((M, 4), dtype=np.int32)
    k = min(count, M)
    first[:k] = firsts[:k]
    label[:k] = lab.reshape(-1)[firsts[:k]]
    sel = live & (ids < k)
    pix = np.nonzero(sel)[0]
    which = ids[pix]
    area[:k] = np.bincount(which, minlength=k)[:k]
    y, x = pix // W, pix % W
    lo = np.full((k, 2), max(H, W), dtype=np.int64)
    hi = np.zeros((k, 2), dtype=np.int64)
    np.minimum.at(lo[:, 0], which, x)
    np.minimum.at(lo[:, 1], which, y)
    np.maximum.at(hi[:, 0], which, x + 1)
    np.maximum.at(hi[:, 1], which, y + 1)
    box[:k, :2] = lo
    box[:k, 2:] = hi
    return ids.reshape(H, W), count, first, label, area, box


def components_host(labels, connectivity=4, ignore=-1, M=256):
    """labels int [B, H, W] -> dict(ids int32 [B,H,W], count int32 [B], first / label / area int32 [B,M], box int32 [B,M,4])"""
    labels = np.asarray(labels)
    out = [components_frame(f, connectivity, ignore, M) for f in labels]
    return {k: np.stack([np.asarray(o[i], dtype=np.int32) for o in out]) for i, k in enumerate(FIELDS)}


def flood_fill(lab, connectivity, ignore):
    """The rule by a naive breadth-first fill from every unvisited pixel in raster order: (ids [H, W], count).  Independent of the
    restatement above; for small maps."""
    lab = np.asarray(lab)
    H, W = lab.shape
    ids = np.full((H, W), -1, dtype=np.int32)
    near = [(0, 1), (0, -1), (1, 0), (-1, 0)] + ([(1, 1), (1, -1), (-1, 1), (-1, -1)] if connectivity == 8 else [])
    count = 0
    for y0 in range(H):
        for x0 in range(W):
            v = lab[y0, x0]
            if ids[y0, x0] >= 0 or v < 0 or v == ignore:
                continue
            ids[y0, x0] = count
            todo = deque([(y0, x0)])
            while todo:
                y, x = todo.popleft()
                for dy, dx in near:
                    yy, xx = y + dy, x + dx
                    if 0 <= yy < H and 0 <= xx < W and ids[yy, xx] < 0 and lab[yy, xx] == v:
                        ids[yy, xx] = count
                        todo.append((yy, xx))
            count += 1
    return ids, count


def discover_host(margin, fg, seed_cell, hp, wp, patch, connectivity=4):
    """DINOSeg.discover from the cut on, on host arrays: margin fp32 [B, n], fg uint8 [B, n], seed_cell int [B] ->
    dict(cells uint8 [B, n], box int32 [B, 4], found uint8 [B], area int32 [B], margin fp32 [B, n] with the cells outside the
    component pushed to -|margin|, grid_labels int32 [B, n] = the labels at the grid's own size)."""
    margin, fg = np.asarray(margin, dtype=np.float32), np.asarray(fg)
    B, n = fg.shape
    comp = components_host(fg.reshape(B, hp, wp).astype(np.int32), connectivity, 0, n)
    cells = np.zeros((B, n), dtype=np.uint8)
    box = np.zeros((B, 4), dtype=np.int32)
    found = np.zeros(B, dtype=np.uint8)
    area = np.zeros(B, dtype=np.int32)
    for b in range(B):
        s = int(seed_cell[b])
        k = int(comp["ids"][b].reshape(-1)[s])
        found[b] = fg[b, s]
        if k >= 0:
            cells[b] = comp["ids"][b].reshape(-1) == k
            box[b] = comp["box"][b, k] * patch
            area[b] = comp["area"][b, k]
    pushed = np.where(cells.astype(bool), margin, -np.abs(margin)).astype(np.float32)
    return dict(cells=cells, box=box, found=found, area=area, margin=pushed, grid_labels=(pushed > 0).astype(np.int32))


# ---- the maps of the device tests
def random_map(seed, H, W, classes=2, p=None, void=0.0):
    """classes = 2: label 1 with probability p; else uniform over the classes; a share `void` of the pixels gets -1 or -7"""
    g = np.random.default_rng(seed)
    m = (g.random((H, W)) < p).astype(np.int32) if p is not None else g.integers(0, classes, (H, W)).astype(np.int32)
    if void:
        holes = g.random((H, W)) < void
        m[holes] = np.where(g.random((H, W)) < 0.5, -1, -7)[holes]
    return m


def checkerboard(H, W):
    return ((np.arange(H)[:, None] + np.arange(W)[None, :]) & 1).astype(np.int32)


def stripes(H, W, vertical):
    return np.array(np.broadcast_to(((np.arange(W)[None, :] if vertical else np.arange(H)[:, None]) & 1), (H, W)), dtype=np.int32, order="C")


def serpentine(H, W):
    """one path one pixel wide through the whole frame (label 1) on void: every other row is full, the rows between hold one pixel at
    alternating ends"""
    m = np.full((H, W), -1, dtype=np.int32)
    m[0::2] = 1
    for i, y in enumerate(range(1, H, 2)):
        m[y, W - 1 if i % 2 == 0 else 0] = 1
    return m


def comb(H, W):
    """a spine along the top row with a tooth down every other column (label 2), label 0 between the teeth"""
    m = np.zeros((H, W), dtype=np.int32)
    m[0] = 2
    m[:, 0::2] = 2
    if H > 1:
        m[H - 1, :] = np.where(np.arange(W) % 2 == 0, 2, 0)
    return m


def corner_pair(H, W, main):
    """two pixels that touch only across the corner where four tiles meet: (31, 63)-(32, 64) or (31, 64)-(32, 63), as (y, x)"""
    m = np.full((H, W), -1, dtype=np.int32)
    if H > 32 and W > 64:
        for y, x in (((31, 63), (32, 64)) if main else ((31, 64), (32, 63))):
            m[y, x] = 5
    else:                                                               # a frame without that corner: the same pair at its own centre
        y, x = H // 2, W // 2
        m[max(y - 1, 0), max(x - 1, 0) if main else x] = 5
        m[y, x if main else max(x - 1, 0)] = 5
    return m
