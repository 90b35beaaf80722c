"""Host restatements for the CLS attention tests, written from the rule in include/dinoseg.h (dinoseg_op_cls_attention):

* the cumulative-mass threshold in exact integers: q_j = rint(p_j 2^30), T = sum q_j, S_le(v) = sum of the q_j <= v,
  t = rint(threshold 2^24) of the fp32 threshold; patch j is kept iff S_le(q_j) 2^24 > (2^24 - t) T (int64: T < 2^31, so every
  product stays below 2^55);
* the nearest gather with exact integer coordinates: pixel (oy, ox) of OH x OW takes patch ((oy hp) // OH, (ox wp) // OW).
"""
import numpy as np


def quantise(p):
    """fp32 probabilities -> int64 q = rint(p 2^30) (the product is exact in fp32: a power-of-two scale)"""
    p = np.asarray(p)
    assert p.dtype == np.float32
    return np.rint(p * np.float32(2.0 ** 30)).astype(np.int64)


def threshold_units(threshold):
    return int(np.rint(np.float64(np.float32(threshold)) * 2.0 ** 24))


def keep_rule(p, threshold):
    """p fp32 [..., n] (the patches of one (frame, head) along the last axis) -> uint8 [..., n]"""
    q = quantise(p)
    t = threshold_units(threshold)
    flat = q.reshape(-1, q.shape[-1])
    out = np.zeros(flat.shape, dtype=np.uint8)
    for r, row in enumerate(flat):
        srt = np.sort(row)
        csum = np.cumsum(srt)                                   # int64, exact
        T = int(csum[-1])
        assert T < 2 ** 31
        s_le = csum[np.searchsorted(srt, row, side="right") - 1]    # the sum of every q <= q_j, ties included
        out[r] = (s_le * 2 ** 24 > (2 ** 24 - t) * T).astype(np.uint8)
    return out.reshape(q.shape)


def sort_rule_fp64(p, threshold):
    """The plain rule: ascending sort, normalise by the row's own sum, keep where the cumulative sum exceeds 1 - threshold; fp64.
    p [n] -> (bool [n], the smallest |cumulative mass - (1 - threshold)| over the row: the margin of the cut)"""
    p = np.asarray(p, dtype=np.float64)
    idx = np.argsort(p, kind="stable")
    cum = np.cumsum(p[idx] / p.sum())
    keep = np.zeros(p.shape, dtype=bool)
    keep[idx] = cum > 1.0 - float(np.float32(threshold))
    return keep, float(np.abs(cum - (1.0 - float(np.float32(threshold)))).min())


def nearest_index(i, o):
    """source index of each of o output positions over i source positions"""
    return (np.arange(o, dtype=np.int64) * i) // o


def nearest_gather(grid, OH, OW):
    """[..., hp, wp] -> [..., OH, OW]"""
    grid = np.asarray(grid)
    sy, sx = nearest_index(grid.shape[-2], OH), nearest_index(grid.shape[-1], OW)
    return grid[..., sy[:, None], sx[None, :]]
