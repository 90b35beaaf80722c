"""The multi-object discovery rule of include/dinoseg.h (dinoseg_op_maskcut) restated in numpy int64 / fp64 on top of tests/ncut_util.py
(the cut) and tests/components_util.py (the component around the seed): the mask, the candidates, the select step, a whole run of K
rounds, the plain matrix form of a round, and the planted grids of the tests."""
import numpy as np

from tests import components_util as CU
from tests import ncut_util as NC

SIGN = np.uint32(0x80000000)

# (hp, wp, D, rectangles as (y0, x0, y1, x1), half-open): the grids on which the planted expectation holds
PLANTED = [
    (5, 7, 64, ((1, 1, 3, 3), (2, 4, 5, 7))),
    (8, 8, 64, ((0, 0, 3, 3), (5, 4, 8, 8))),
    (5, 13, 64, ((0, 0, 2, 3), (3, 9, 5, 13))),
    (9, 11, 192, ((1, 1, 4, 4), (5, 1, 8, 5), (1, 6, 5, 10))),
]


# ---- alive: one bit per cell ---------------------------------------------------------------------------------------------------
def pack_alive(alive):
    """bool [n] -> uint64 [ceil(n / 64)]: cell i at bit i % 64 of word i // 64, pad bits zero"""
    return NC.pack_bits(np.asarray(alive, dtype=bool)[None, :])[0]


def unpack_alive(words, n):
    """uint64 [W] -> (bool [n], bool [64 W - n] the pad bits)"""
    bits, pad = NC.unpack_words(np.asarray(words).reshape(1, -1), n)
    return bits[0], pad[0]


# ---- step 1: the mask ----------------------------------------------------------------------------------------------------------
def mask_host(words, alive_words):
    """words uint64 [n, W], alive_words uint64 [W] -> (the masked words [n, W], degree int64 [n]): row i <- alive_i ? row i & alive : 0"""
    words = np.ascontiguousarray(words).astype(np.uint64)
    n = words.shape[0]
    alive, _ = unpack_alive(alive_words, n)
    out = np.where(alive[:, None], words & np.asarray(alive_words, dtype=np.uint64)[None, :], np.uint64(0))
    degree = np.unpackbits(out.view(np.uint8), axis=1).sum(1).astype(np.int64)
    return out, degree


# ---- steps 3 and 4: the candidates and the select ----------------------------------------------------------------------------------
def candidates_host(fg, alive):
    return ((np.asarray(fg) != 0) & np.asarray(alive, dtype=bool)).astype(np.int32)


def pushed_bits(margin, cells):
    """the bits of where(cells, margin, -|margin|) as uint32: margin with the sign bit set outside the cells"""
    m = np.ascontiguousarray(margin, dtype=np.float32).view(np.uint32)
    return np.where(np.asarray(cells, dtype=bool), m, m | SIGN)


def select_host(ids, fg, margin, seed, alive, hp, wp):
    """ids int [n] (-1 on void cells), fg [n], margin fp32 [n], the seed cell, alive bool [n] -> dict(found, k, cells bool [n], area,
    box (x0, y0, x1, y1) in cells, alive bool [n] after the round, score uint32 [n]: the bits of the round's channel)"""
    ids, fg, alive = np.asarray(ids).reshape(-1), np.asarray(fg).reshape(-1), np.asarray(alive, dtype=bool)
    n, s = hp * wp, int(seed)
    k = int(ids[s]) if 0 <= s < n and alive[s] and fg[s] != 0 else -1
    found = k >= 0
    cells = (ids == k) if found else np.zeros(n, dtype=bool)
    box = np.zeros(4, dtype=np.int32)
    if found:
        at = np.nonzero(cells)[0]
        y, x = at // wp, at % wp
        box[:] = (x.min(), y.min(), x.max() + 1, y.max() + 1)
    return dict(found=int(found), k=k, cells=cells, area=int(cells.sum()), box=box, alive=alive & ~cells, score=pushed_bits(margin, cells))


# ---- a whole run in fp64 -------------------------------------------------------------------------------------------------------
def round_host(bits, alive, hp, wp, eps, start, iters, connectivity=4):
    """One round on the ORIGINAL graph bool [n, n] and the state alive bool [n]: the mask through the packed words, the cut by
    NC.iterate_host / NC.result_host on the masked graph with n the full cell count, the component around the seed ->
    dict(masked bool [n, n], degree, z, rho, res = the result rule's dict, ids, + the fields of select_host)"""
    n = hp * wp
    words, degree = mask_host(NC.pack_bits(bits), pack_alive(alive))
    masked, pad = NC.unpack_words(words, n)
    assert not pad.any()
    _, r, u = NC.weights(degree, n, eps)
    z, rho = NC.iterate_host(masked.astype(np.float64), r, u, eps, start, iters)
    res = NC.result_host(z, r)
    cand = candidates_host(res["fg"], alive)
    ids = CU.components_frame(cand.reshape(hp, wp), connectivity, 0, 1)[0].reshape(-1)
    out = dict(masked=masked, degree=degree, z=z, rho=rho, res=res, ids=ids)
    out.update(select_host(ids, res["fg"], res["margin"].astype(np.float32), res["seed"], alive, hp, wp))
    return out


def maskcut_host(bits, hp, wp, eps, start, iters, K, connectivity=4):
    """K rounds from every cell alive -> (the rounds' dicts, count, grid_labels int32 [n]: the argmax over (0, the rounds' channels) with
    the first maximum, the labels at the grid's own size)"""
    n = hp * wp
    alive, rounds = np.ones(n, dtype=bool), []
    for _ in range(K):
        rounds.append(round_host(bits, alive, hp, wp, eps, start, iters, connectivity))
        alive = rounds[-1]["alive"]
    score = np.stack([np.zeros(n, dtype=np.float32)] + [r["score"].view(np.float32) for r in rounds], axis=1)
    return rounds, sum(r["found"] for r in rounds), np.argmax(score, axis=1).astype(np.int32)


def matrix_round(bits, alive, eps, start, iters):
    """The plain matrix form of a round's cut: the dense W = eps 11^T + (1 - eps) Bits of the ORIGINAL graph with the rows and columns of
    the dead cells set to eps, fed to NC.matrix_form -> (z, rho)"""
    n = bits.shape[0]
    dead = ~np.asarray(alive, dtype=bool)
    Wm = eps * np.ones((n, n)) + (1.0 - eps) * bits.astype(np.float64)
    Wm[dead, :] = eps
    Wm[:, dead] = eps
    joined = (Wm - eps) / (1.0 - eps)                                   # what NC.matrix_form turns back into this W
    _, r, u = NC.weights(np.rint(joined).sum(1), n, eps)
    z, rho, _ = NC.matrix_form(joined, r, u, eps, start, iters)
    return z, rho


# ---- planted grids -------------------------------------------------------------------------------------------------------------
def rect_cells(hp, wp, rects):
    """the rectangles' cell sets bool [G, n] and the object map int32 [n]: g + 1 inside rectangle g, 0 on the background"""
    sets = np.zeros((len(rects), hp, wp), dtype=bool)
    for g, (y0, x0, y1, x1) in enumerate(rects):
        sets[g, y0:y1, x0:x1] = True
    sets = sets.reshape(len(rects), hp * wp)
    assert sets.sum(0).max() <= 1, "the rectangles overlap"
    return sets, (sets * np.arange(1, len(rects) + 1)[:, None]).sum(0).astype(np.int32)


def planted_rect_tokens(seed, hp, wp, D, rects, noise=0.5, scale=3.0):
    """Orthogonal unit directions, one per rectangle and one for the background; every cell = scale (its direction + noise x a unit
    noise row) -> tokens fp32 [1 + n, D] with a CLS row in front"""
    rng = np.random.default_rng(seed)
    n, G = hp * wp, len(rects)
    dirs = np.linalg.qr(rng.standard_normal((D, G + 1)))[0].T           # [G + 1, D], orthonormal rows
    which = rect_cells(hp, wp, rects)[1]
    x = dirs[which] + noise * NC.unit_rows(rng.standard_normal((n, D)))
    tok = np.empty((n + 1, D), dtype=np.float32)
    tok[0] = rng.standard_normal(D).astype(np.float32)
    tok[1:] = (scale * x).astype(np.float32)
    return tok


def host_bits(tok, tau=0.2):
    """tokens [1 + n, D] -> the graph bool [n, n] of their unit rows in fp64 at tau rounded to fp32"""
    X = NC.unit_rows(np.asarray(tok, dtype=np.float64)[1:])
    return NC.scores_host(X) > float(np.float32(tau))


def found_sets(cells, found):
    """the rounds' cell sets as a set of frozensets of cell indices, not-found rounds left out"""
    return {frozenset(np.nonzero(np.asarray(c))[0].tolist()) for c, f in zip(cells, found) if f}


def rect_sets(hp, wp, rects):
    return {frozenset(np.nonzero(s)[0].tolist()) for s in rect_cells(hp, wp, rects)[0]}
