"""Yardsticks of the image-guided upsample (include/dinoseg.h, dinoseg_op_upsample_guided).

``guided_ref`` restates the rule in exact integers (cells, my, D) and fp64 (everything else), with the fp32-rounded constants the
library uses, vectorised over the pixels.  ``jbu_plain`` is a second, independent statement of joint bilateral upsampling in plain
loops -- floating-point pixel coordinates, no Dmin -- against which the first is checked on tiny shapes in the CPU suite.
"""
import math

import numpy as np

LOG2E = 1.44269504088896340736


def guided_constants(sigma_spatial, sigma_range):
    """(a_s, a_r): computed in fp64, rounded once to fp32 (returned as the fp64 value of that fp32)."""
    a_s = np.float32(LOG2E / (2.0 * float(sigma_spatial) ** 2))
    a_r = np.float32(LOG2E / (2.0 * (255.0 * float(sigma_range)) ** 2))
    return float(a_s), float(a_r)


def cell_colours(guide, hp, wp):
    """guide uint8 [B, OH, OW, 3] -> int64 [B, hp, wp, 3]: the rounded mean (2 sum + n) // (2 n) over each cell's pixels, pixel
    (y, x) belonging to cell ((y hp) // OH, (x wp) // OW)."""
    B, OH, OW, _ = guide.shape
    ry = (np.arange(OH, dtype=np.int64) * hp) // OH
    rx = (np.arange(OW, dtype=np.int64) * wp) // OW
    cell = (ry[:, None] * wp + rx[None, :]).reshape(-1)
    n = np.bincount(cell, minlength=hp * wp).astype(np.int64)
    out = np.empty((B, hp * wp, 3), dtype=np.int64)
    g = guide.reshape(B, OH * OW, 3).astype(np.int64)
    for b in range(B):
        for ch in range(3):
            s = np.bincount(cell, weights=g[b, :, ch], minlength=hp * wp)       # (sums < 2^53: exact in the fp64 weights)
            out[b, :, ch] = (2 * s.astype(np.int64) + n) // (2 * n)
    return out.reshape(B, hp, wp, 3)


def pack_cells(colours):
    """int64 [B, hp, wp, 3] -> uint32 [B, hp, wp] packed R | G << 8 | B << 16."""
    return (colours[..., 0] | (colours[..., 1] << 8) | (colours[..., 2] << 16)).astype(np.uint32)


def guided_ref(logp, guide, hp, wp, radius, sigma_spatial, sigma_range):
    """logp [B, hp*wp, C], guide uint8 [B, OH, OW, 3] -> dense fp64 [B, C, OH, OW] by the rule of include/dinoseg.h."""
    B, OH, OW, _ = guide.shape
    C = logp.shape[-1]
    R = int(radius)
    a_s, a_r = guided_constants(sigma_spatial, sigma_range)
    L = np.asarray(logp, dtype=np.float64).reshape(B, hp, wp, C)
    col = cell_colours(guide, hp, wp)
    g = guide.astype(np.int64)
    oy = np.arange(OH, dtype=np.int64)
    ox = np.arange(OW, dtype=np.int64)
    r0, c0 = (oy * hp) // OH, (ox * wp) // OW
    taps = [(dr, dc) for dr in range(-R, R + 1) for dc in range(-R, R + 1)]
    big = np.int64(1) << 40

    def tap(dr, dc):
        r, c = r0 + dr, c0 + dc
        ok = ((r >= 0) & (r < hp))[:, None] & ((c >= 0) & (c < wp))[None, :]
        rc, cc = np.clip(r, 0, hp - 1), np.clip(c, 0, wp - 1)
        d = g - col[:, rc][:, :, cc]                                            # [B, OH, OW, 3]
        D = (d * d).sum(-1)
        my = 2 * r * OH - ((2 * oy + 1) * hp - OH)
        mx = 2 * c * OW - ((2 * ox + 1) * wp - OW)
        dy, dx = my.astype(np.float64) / float(2 * OH), mx.astype(np.float64) / float(2 * OW)
        s = (dy * dy)[:, None] + (dx * dx)[None, :]
        return ok, rc, cc, D, s

    Dmin = np.full((B, OH, OW), big, dtype=np.int64)
    for dr, dc in taps:
        ok, _, _, D, _ = tap(dr, dc)
        Dmin = np.minimum(Dmin, np.where(ok[None], D, big))
    acc = np.zeros((B, OH, OW, C), dtype=np.float64)
    W = np.zeros((B, OH, OW), dtype=np.float64)
    for dr, dc in taps:
        ok, rc, cc, D, s = tap(dr, dc)
        w = np.where(ok[None], np.exp2(-(s[None] * a_s) - (D - Dmin).astype(np.float64) * a_r), 0.0)
        acc += w[..., None] * L[:, rc][:, :, cc]
        W += w
    return np.ascontiguousarray((acc / W[..., None]).transpose(0, 3, 1, 2))


def first_argmax_and_margin(dense):
    """dense [B, C, OH, OW] -> (the first maximum over C, the top-2 margin; inf with one class)."""
    lab = dense.argmax(1)
    if dense.shape[1] == 1:
        return lab, np.full(lab.shape, np.inf)
    top = np.partition(dense, dense.shape[1] - 2, axis=1)
    return lab, top[:, -1] - top[:, -2]


def nearest_ref(logp, hp, wp, OH, OW):
    """The nearest-neighbour enlargement of logp [B, hp*wp, C] -> [B, C, OH, OW] (same dtype: a gather)."""
    B, C = logp.shape[0], logp.shape[-1]
    r0, c0 = (np.arange(OH) * hp) // OH, (np.arange(OW) * wp) // OW
    return np.ascontiguousarray(logp.reshape(B, hp, wp, C)[:, r0][:, :, c0].transpose(0, 3, 1, 2))


def jbu_plain(logp, guide, hp, wp, radius, sigma_spatial, sigma_range):
    """Joint bilateral upsampling in plain loops: per pixel, over the cells within `radius` of the cell the pixel falls in, the
    mean of the cells' values weighted by a Gaussian of the distance between the pixel's align_corners=False coordinate and the
    cell's index, times a Gaussian of the colour distance between the pixel and the cell's (rounded mean) colour."""
    B, OH, OW, _ = guide.shape
    C = logp.shape[-1]
    a_s, a_r = guided_constants(sigma_spatial, sigma_range)
    # cell colours by plain loops
    col = [[[None] * wp for _ in range(hp)] for _ in range(B)]
    for b in range(B):
        sums = [[[0, 0, 0, 0] for _ in range(wp)] for _ in range(hp)]
        for y in range(OH):
            for x in range(OW):
                e = sums[(y * hp) // OH][(x * wp) // OW]
                for ch in range(3):
                    e[ch] += int(guide[b, y, x, ch])
                e[3] += 1
        for r in range(hp):
            for c in range(wp):
                s0, s1, s2, n = sums[r][c]
                col[b][r][c] = tuple((2 * s + n) // (2 * n) for s in (s0, s1, s2))
    out = np.zeros((B, C, OH, OW), dtype=np.float64)
    for b in range(B):
        for y in range(OH):
            py = (y + 0.5) * hp / OH - 0.5
            ry = (y * hp) // OH
            for x in range(OW):
                px = (x + 0.5) * wp / OW - 0.5
                rx = (x * wp) // OW
                pix = [int(v) for v in guide[b, y, x]]
                acc, wsum = [0.0] * C, 0.0
                for r in range(max(ry - radius, 0), min(ry + radius, hp - 1) + 1):
                    for c in range(max(rx - radius, 0), min(rx + radius, wp - 1) + 1):
                        d2 = (py - r) ** 2 + (px - c) ** 2
                        D = sum((p - q) ** 2 for p, q in zip(pix, col[b][r][c]))
                        w = math.pow(2.0, -d2 * a_s) * math.pow(2.0, -D * a_r)
                        wsum += w
                        for k in range(C):
                            acc[k] += w * float(logp[b, r * wp + c, k])
                for k in range(C):
                    out[b, k, y, x] = acc[k] / wsum
    return out


def log_softmax(z):
    z = np.asarray(z, dtype=np.float64)
    m = z.max(-1, keepdims=True)
    return z - m - np.log(np.exp(z - m).sum(-1, keepdims=True))


def make_logp(rng, B, hp, wp, C):
    """log_softmax(3 randn), fp32 [B, hp*wp, C]."""
    return log_softmax(3.0 * rng.standard_normal((B, hp * wp, C))).astype(np.float32)


def make_guides(rng, B, OH, OW):
    """Two guides: uniform random bytes, and random 5 x 7-pixel blocks of one colour."""
    noise = rng.integers(0, 256, size=(B, OH, OW, 3), dtype=np.uint8)
    by, bx = (OH + 4) // 5, (OW + 6) // 7
    blocks = rng.integers(0, 256, size=(B, by, bx, 3), dtype=np.uint8)
    blocks = np.repeat(np.repeat(blocks, 5, axis=1), 7, axis=2)[:, :OH, :OW]
    return noise, np.ascontiguousarray(blocks)


def edge_case(e, vertical):
    """The edge-following construction: 4 x 6 cells under 32 x 48 pixels, a two-colour guide whose edge lies at column e, and
    two-class log-probs that put every cell on the side its centre lies on; the horizontal edge is the transpose (6 x 4 cells under
    48 x 32 pixels, the edge at row e), so that every e has cells on both sides.  Returns (logp fp32 [1, hp*wp, 2], guide, the
    expected labels [1, OH, OW], hp, wp)."""
    hp, wp, OH, OW = (4, 6, 32, 48) if vertical else (6, 4, 48, 32)
    yy, xx = np.mgrid[0:OH, 0:OW]
    right = (xx >= e) if vertical else (yy >= e)
    guide = np.where(right[..., None], np.array([30, 30, 200]), np.array([200, 30, 30])).astype(np.uint8)[None]
    lo, hi = log_softmax([2.0, 0.0]), log_softmax([0.0, 2.0])
    logp = np.empty((hp, wp, 2), dtype=np.float64)
    for r in range(hp):
        for c in range(wp):
            centre = (c + 0.5) * OW / wp if vertical else (r + 0.5) * OH / hp
            logp[r, c] = hi if centre >= e else lo
    return logp.reshape(1, hp * wp, 2).astype(np.float32), np.ascontiguousarray(guide), right.astype(np.int64)[None], hp, wp


def value_bar(radius, logp):
    """(16 + 2 T) 2^-24 max|logp|, T = (2R+1)^2: one product and one add of same-sign values per tap (2 T), and 16 units for the
    weights' own error (x 2^-x <= 0.54 bounds what an exponent's rounding can move a weight that matters), the reciprocal, the
    final product and the contraction order."""
    T = (2 * int(radius) + 1) ** 2
    return (16 + 2 * T) * 2.0 ** -24 * float(np.abs(logp).max())
