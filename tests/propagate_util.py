"""The label-propagation rule of include/dinoseg.h (dinoseg_op_propagate, dinoseg_op_label_cells) restated in int64 / fp64 numpy:
the context schedule, unit rows, candidates and the selection under the total order (score descending, global index ascending),
weights and value, the seed rule, and the test that says whether a query's selection is decided at the scores' error bar."""
import numpy as np

LOG2E = 1.4426950408889634074


def context_frames(t, n_context):
    """frame 0 first, then the last min(t - 1, n_context) frames before t, oldest first"""
    assert t >= 1 and n_context >= 0
    return [0] + list(range(max(1, t - n_context), t))


def unit_rows(f):
    """f^ = f / max(||f||_2, 1e-12) in fp64; f [..., D]"""
    f = np.asarray(f, dtype=np.float64)
    return f / np.maximum(np.sqrt((f * f).sum(-1, keepdims=True)), 1e-12)


def score_bar(D):
    """E(D) = (D + 16) 2^-24: the worst-case fp32 accumulation bound for unit vectors (sum |a_i b_i| <= 1) plus the plane split"""
    return (D + 16) * 2.0 ** -24


def value_bar(D, k, tau, seg_max):
    """(4 E / tau + (16 + 2k) 2^-24) max|seg|: each selected weight is off by at most 2E / tau relative, which doubles through the
    normalisation; the last term covers the fmaf chain"""
    return (4.0 * score_bar(D) / tau + (16 + 2 * k) * 2.0 ** -24) * seg_max


def neighbours(hp, wp, R):
    """per query cell the candidate cells of ONE context frame: (index int64 [n, S], valid bool [n, S]) with S = (2 R' + 1)^2, R' the
    radius clipped to the grid; candidates of a query in ascending cell index"""
    Rc = min(int(R), max(hp, wp) - 1)
    r, c = np.divmod(np.arange(hp * wp, dtype=np.int64), wp)
    d = np.arange(-Rc, Rc + 1, dtype=np.int64)
    rr = r[:, None, None] + d[None, :, None]
    cc = c[:, None, None] + d[None, None, :]
    valid = (rr >= 0) & (rr < hp) & (cc >= 0) & (cc < wp)
    idx = np.where(valid, rr * wp + cc, 0)
    return idx.reshape(hp * wp, -1), valid.reshape(hp * wp, -1)


def ranked_candidates(ft, fctx, hp, wp, R):
    """All candidates of every query in the total order.  ft [n, D] raw target rows, fctx [n_ctx, n, D] raw context rows ->
    (scores fp64 [n, M] descending, -inf beyond the count; g int64 [n, M], -1 beyond; count int64 [n])"""
    n = hp * wp
    qt, kc = unit_rows(ft), unit_rows(fctx)
    idx, valid = neighbours(hp, wp, R)
    s_all, g_all = [], []
    for ci in range(kc.shape[0]):
        S = qt @ kc[ci].T                                             # [n, n] fp64
        s_all.append(np.where(valid, np.take_along_axis(S, idx, axis=1), -np.inf))
        g_all.append(np.where(valid, ci * n + idx, np.iinfo(np.int64).max))
    s, g = np.concatenate(s_all, axis=1), np.concatenate(g_all, axis=1)
    s = s + 0.0                                                         # (-0 is +0)
    order = np.lexsort((g, -s), axis=-1)                                # primary: score descending; then g ascending
    s, g = np.take_along_axis(s, order, axis=1), np.take_along_axis(g, order, axis=1)
    count = np.isfinite(s).sum(axis=1)
    return s, np.where(np.isfinite(s), g, -1), count


def scale_a(tau):
    """a = log2(e) / tau in fp64, rounded once to fp32"""
    return float(np.float32(LOG2E / float(tau)))


def weights_and_value(s_sel, g_sel, segs, tau):
    """Steps 4 and 5 in fp64 for selections in rank order.  s_sel fp64 [n, k], g_sel int64 [n, k] (-1 beyond K'), segs [n_ctx, n, C]
    -> (w / W fp64 [n, k], 0 beyond K'; V fp64 [n, C])"""
    segs = np.asarray(segs, dtype=np.float64)
    flat = segs.reshape(-1, segs.shape[-1])
    ok = g_sel >= 0
    w = np.where(ok, np.exp2((np.where(ok, s_sel, 0.0) - s_sel[:, :1]) * scale_a(tau)), 0.0)
    W = w.sum(axis=1, keepdims=True)
    V = np.einsum("qk,qkc->qc", w, flat[np.where(ok, g_sel, 0)]) / W
    return w / W, V


def propagate_host(ft, fctx, segs, hp, wp, R, k, tau):
    """The whole rule for one target frame: (topk g int64 [n, k] in rank order with -1 beyond K', w / W [n, k], V [n, C], and the ranked
    candidates (scores, g, count) the decision test reads)"""
    s, g, count = ranked_candidates(ft, fctx, hp, wp, R)
    kk = min(k, s.shape[1])
    s_sel = np.full((s.shape[0], k), -np.inf)
    g_sel = np.full((s.shape[0], k), -1, dtype=np.int64)
    s_sel[:, :kk], g_sel[:, :kk] = s[:, :kk], g[:, :kk]
    wn, V = weights_and_value(s_sel, g_sel, segs, tau)
    return g_sel, wn, V, (s, g, count)


def decided(ranked, k, E):
    """bool [n]: the fp64 gap at the cut, s_(K'-1) - s_(K'), exceeds 2E; a query with #candidates <= k is always decided"""
    s, _, count = ranked
    out = count <= k
    if s.shape[1] > k:
        out = out | ((s[:, k - 1] - s[:, k]) > 2.0 * E)
    return out


def scores_of(ft, fctx, g_sel):
    """the fp64 scores of given selections: g_sel int64 [n, k] (-1: none) -> fp64 [n, k] (-inf where none)"""
    n = ft.shape[0]
    qt, kc = unit_rows(ft), unit_rows(fctx).reshape(-1, ft.shape[1])
    ok = g_sel >= 0
    s = np.einsum("qd,qkd->qk", qt, kc[np.where(ok, g_sel, 0)]) + 0.0
    assert g_sel.shape[0] == n
    return np.where(ok, s, -np.inf)


def label_cells_host(labels, hp, wp, C):
    """The seed rule: integer pixel labels [OH, OW] -> fp32 [n, C]; pixel (y, x) belongs to cell ((y hp) // OH, (x wp) // OW);
    seg[cell, c] = float32(count_c) / float32(n_cell); labels outside [0, C) count in n_cell and in no class"""
    y = np.asarray(labels).astype(np.int64)
    OH, OW = y.shape
    cr = (np.arange(OH, dtype=np.int64) * hp) // OH
    cc = (np.arange(OW, dtype=np.int64) * wp) // OW
    cell = (cr[:, None] * wp + cc[None, :]).reshape(-1)
    y = y.reshape(-1)
    n_cell = np.bincount(cell, minlength=hp * wp).astype(np.int64)
    counts = np.zeros((hp * wp, C), dtype=np.int64)
    ok = (y >= 0) & (y < C)
    np.add.at(counts, (cell[ok], y[ok]), 1)
    return counts.astype(np.float32) / n_cell.astype(np.float32)[:, None]


def make_case(seed, hp, wp, D, C, n_ctx):
    """one seed per case: unnormalised Gaussian rows (target tokens with a CLS row, context tokens likewise) and softmax segs"""
    rng = np.random.default_rng(seed)
    n = hp * wp
    tok_t = rng.standard_normal((1, n + 1, D)).astype(np.float32)
    tok_c = rng.standard_normal((n_ctx, n + 1, D)).astype(np.float32)
    z = rng.standard_normal((n_ctx, n, C)) * 2.0
    e = np.exp(z - z.max(-1, keepdims=True))
    segs = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    return tok_t, tok_c, segs
