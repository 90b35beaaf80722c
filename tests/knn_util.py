"""The k-NN label retrieval rule of include/dinoseg.h (dinoseg_op_knn_labels) restated in int64 / fp64 numpy: the planes' defined
value, the bank's split ranges, the selection under the total order (score descending, bank row ascending), weights and value for
both label kinds, and the builders of the test cases.  Nothing here launches a kernel."""
import numpy as np

from tests import propagate_util as P

TAU = 0.1
MAX_SPLITS = 16
SOFT, HARD = 0, 1
VOID = 255

# (B, n, M, bank_rows, D, C, k, kind): the cases of the device test, one seed each
CASES = [
    (1, 1, 1, 1, 64, 2, 1, SOFT),               # the smallest problem
    (1, 35, 3, 64, 64, 3, 5, SOFT),             # K' = M < k, dead rows behind M
    (2, 35, 65, 65, 64, 7, 5, HARD),            # a query tile spans two frames, a ragged key block, some rows void
    (1, 64, 129, 200, 192, 5, 16, SOFT),        # k at its limit
    (2, 480, 5000, 5000, 384, 150, 5, SOFT),    # a mid-size soft bank
    (1, 192, 1000, 1024, 768, 256, 1, HARD),    # ViT-B width at the class limit
    (1, 4800, 4096, 4096, 384, 7, 5, HARD),     # the camera's grid, once
]
SEEDS = [400, 401, 402, 403, 404, 405, 406]


def case_id(i):
    return "x".join(str(v) for v in CASES[i])


# ---- the planes ---------------------------------------------------------------------------------------------------------------
def split_rows(f):
    """dinoseg_op_normalize_tokens on the host: raw rows [..., rows, D] -> fp16 planes [..., 2, rows, D], 2^10 f^ = hi + lo with
    hi = fp16(fp32(v)), lo = fp16(fp32(v - hi)), the norm and the quotient in fp64"""
    v = P.unit_rows(f) * 1024.0
    hi = v.astype(np.float32).astype(np.float16)
    lo = (v - hi.astype(np.float64)).astype(np.float32).astype(np.float16)
    return np.ascontiguousarray(np.stack([hi, lo], axis=-3))


def plane_rows(planes):
    """the DEFINED rows of planes [..., 2, rows, D]: (hi + lo) 2^-10 in fp64, [..., rows, D]"""
    p = np.asarray(planes).astype(np.float64)
    return (p[..., 0, :, :] + p[..., 1, :, :]) * 2.0 ** -10


def query_rows(qplanes):
    """[B, 2, n, D] -> fp64 [B n, D]: query i = frame i // n, cell i % n"""
    q = plane_rows(qplanes)
    return q.reshape(-1, q.shape[-1])


# ---- the split ranges ---------------------------------------------------------------------------------------------------------
def split_cap(M, k):
    return min(MAX_SPLITS, 256 // k, (M + 63) // 64)


def library_splits(N, M, k):
    """dinoseg_knn_splits as the header states it"""
    tiles, nblk = (N + 63) // 64, (M + 63) // 64
    return min(split_cap(M, k), max(1, min((512 + tiles - 1) // tiles, nblk // 4)))


def split_ranges(M, S):
    """the rows [first, last + 1) of range s = 0 .. S-1: key blocks floor(s nblk / S) .. floor((s + 1) nblk / S) - 1, clipped at M"""
    nblk = (M + 63) // 64
    return [(64 * ((s * nblk) // S), min(64 * (((s + 1) * nblk) // S), M)) for s in range(S)]


# ---- the rule -----------------------------------------------------------------------------------------------------------------
def label_rows(labels, kind, C):
    """the label store as fp64 rows [rows, C]: soft rows as they are; a hard label is its one-hot row, all zero when void (>= C)"""
    if kind == SOFT:
        return np.asarray(labels, dtype=np.float64)
    return (np.asarray(labels).astype(np.int64)[:, None] == np.arange(C)[None, :]).astype(np.float64)


def ranked(q, bank, M):
    """every live row in the total order: (scores fp64 [N, M] descending, g int64 [N, M], count int64 [N]), P.ranked_candidates' form"""
    s = q @ bank[:M].T + 0.0                                            # (-0 is +0)
    order = np.argsort(-s, axis=1, kind="stable")                       # score descending; a stable sort keeps g ascending on a tie
    return np.take_along_axis(s, order, axis=1), order.astype(np.int64), np.full(q.shape[0], M, dtype=np.int64)


def knn_host(qplanes, bplanes, M, labels, kind, C, k, tau):
    """The whole rule from the planes: (topk g int64 [N, k] in rank order with -1 beyond K', w / W [N, k], V [N, C], and the ranked
    candidates (scores, g, count) that P.decided reads)"""
    q, bank = query_rows(qplanes), plane_rows(bplanes)
    s, g, count = ranked(q, bank, M)
    kk = min(k, M)
    s_sel = np.full((q.shape[0], k), -np.inf)
    g_sel = np.full((q.shape[0], k), -1, dtype=np.int64)
    s_sel[:, :kk], g_sel[:, :kk] = s[:, :kk], g[:, :kk]
    wn, V = P.weights_and_value(s_sel, g_sel, label_rows(labels, kind, C)[None], tau)
    return g_sel, wn, V, (s, g, count)


def scores_of(q, bank, g_sel):
    """the fp64 scores of given selections: g_sel int64 [N', k] (-1: none) for the queries q [N', D] -> fp64 [N', k]"""
    ok = g_sel >= 0
    s = np.einsum("qd,qkd->qk", q, bank[np.where(ok, g_sel, 0)]) + 0.0
    return np.where(ok, s, -np.inf)


# ---- the cases ----------------------------------------------------------------------------------------------------------------
def make_case(i):
    """seeded normal rows, as propagate_util.make_case: (query tokens fp32 [B, n + 1, D] with a CLS row, bank tokens fp32 [1,
    bank_rows + 1, D] likewise, labels: soft fp32 [bank_rows, C] softmax rows, or hard uint8 [bank_rows] with one row in eight void)"""
    B, n, M, rows, D, C, k, kind = CASES[i]
    rng = np.random.default_rng(SEEDS[i])
    tok_q = rng.standard_normal((B, n + 1, D)).astype(np.float32)
    tok_b = rng.standard_normal((1, rows + 1, D)).astype(np.float32)
    if kind == SOFT:
        z = rng.standard_normal((rows, C)) * 2.0
        e = np.exp(z - z.max(-1, keepdims=True))
        labels = (e / e.sum(-1, keepdims=True)).astype(np.float32)
    else:
        labels = rng.integers(0, C, rows).astype(np.uint8)
        labels[rng.random(rows) < 0.125] = VOID if C <= VOID else 0     # (at C = 256 no uint8 value is void)
    return tok_q, tok_b, labels


def host_planes(i):
    """a case's planes by the host's split: (query planes [B, 2, n, D], bank planes [2, bank_rows, D])"""
    tok_q, tok_b, _ = make_case(i)
    return split_rows(tok_q[:, 1:]), split_rows(tok_b[0, 1:])
