"""The spherical k-means rule of include/dinoseg.h (dinoseg_op_kmeans_assign and its neighbours) restated in int64 / fp64 numpy:
points and centroids as the values their fp16 hi + lo planes hold, the assignment with the lowest index on a tie, the update with
kept empty clusters, the records, the error bars, and the test that says whether a point's assignment is decided at the scores' bar."""
import numpy as np

MAX_RANGES, MIN_RANGES, RANGE_WGS, RANGE_MIN = 64, 16, 4096, 256


def score_bar(D):
    """E(D) = (D + 16) 2^-24, the bar of the three-product fp16 MFMA score (tests/propagate_util.py: score_bar)"""
    return (D + 16) * 2.0 ** -24


def plane_values(planes):
    """planes fp16 [..., 2, rows, D] (hi, lo; scaled by 2^10) -> the rows they DEFINE, fp64 [..., rows, D] = (hi + lo) 2^-10"""
    p = np.asarray(planes).astype(np.float64)
    return (p[..., 0, :, :] + p[..., 1, :, :]) * 2.0 ** -10


def points_of(planes):
    """point planes fp16 [B, 2, n, D] -> X fp64 [B n, D], point i = frame i // n, cell i % n"""
    x = plane_values(planes)
    return x.reshape(-1, x.shape[-1])


def split_planes(c32):
    """the planes of an fp32 row: 2^10 c = hi + lo, hi = fp16(2^10 c), lo = fp16(2^10 c - hi); fp32 [K, D] -> fp16 [2, K, D]"""
    v = np.asarray(c32, dtype=np.float32).astype(np.float64) * 1024.0
    hi = v.astype(np.float32).astype(np.float16)
    lo = (v - hi.astype(np.float64)).astype(np.float32).astype(np.float16)
    return np.stack([hi, lo])


def unit_rows(rows):
    """row / max(||row||_2, 1e-12) in fp64"""
    r = np.asarray(rows, dtype=np.float64)
    return r / np.maximum(np.sqrt((r * r).sum(-1, keepdims=True)), 1e-12)


def assign_host(X, C):
    """X fp64 [N, D], C fp64 [K, D] -> (a int64 [N] = argmax_j <x_i, c_j> with the lowest j on a tie, best fp64 [N], gap fp64 [N] between
    the two best scores (inf for K = 1), S fp64 [N, K])"""
    S = X @ C.T + 0.0
    a = np.argmax(S, axis=1)                                            # (numpy returns the first maximum)
    best = S[np.arange(S.shape[0]), a]
    if S.shape[1] == 1:
        gap = np.full(S.shape[0], np.inf)
    else:
        top2 = np.partition(S, S.shape[1] - 2, axis=1)[:, -2:]
        gap = top2[:, 1] - top2[:, 0]
    return a.astype(np.int64), best, gap, S


def update_host(X, a, C_prev):
    """The update in fp64: (C fp64 [K, D] with the previous row where n_j = 0 or ||m_j|| = 0, counts int64 [K], m fp64 [K, D],
    abs_sum fp64 [K, D] = sum over the members of |x_i[d]|, kept bool [K])"""
    K, D = C_prev.shape
    m, A = np.zeros((K, D)), np.zeros((K, D))
    np.add.at(m, a, X)
    np.add.at(A, a, np.abs(X))
    counts = np.bincount(a, minlength=K).astype(np.int64)
    norm = np.sqrt((m * m).sum(-1))
    kept = (counts == 0) | (norm == 0.0)
    C = np.where(kept[:, None], C_prev, m / np.where(kept, 1.0, norm)[:, None])
    return C, counts, m, A, kept


def lloyd_host(X, C0, iters):
    """iters times (assign, update), then the final assignment: (a [N], C [K, D], counts [K], objective [iters + 1], moved [iters + 1])"""
    C, prev, counts = np.array(C0, dtype=np.float64), None, np.zeros(C0.shape[0], dtype=np.int64)
    objective, moved = [], []
    for t in range(iters + 1):
        a, best, _, _ = assign_host(X, C)
        objective.append(best.sum())
        moved.append(X.shape[0] if prev is None else int((a != prev).sum()))
        prev = a
        if t < iters:
            C, counts = update_host(X, a, C)[:2]
    return prev, C, counts, np.array(objective), np.array(moved, dtype=np.int64)


def sum_bar(counts, abs_sum):
    """(n_j + 16) 2^-24 sum_i |x_i[d]|: the worst case of an fp32 sum of n_j terms in any order; [K, D]"""
    return (counts[:, None] + 16) * 2.0 ** -24 * abs_sum


def centroid_bar(m, delta):
    """The bar on c = fp32(m' / ||m'||) for |m' - m| <= delta elementwise (m, delta fp64 [K, D]; rows with ||m|| <= ||delta|| get inf):
    |m'_d / ||m'|| - m_d / ||m||| <= delta_d / ||m'|| + |m_d| | ||m'|| - ||m|| | / (||m'|| ||m||), with | ||m'|| - ||m|| | <= ||delta||
    and ||m'|| >= ||m|| - ||delta||; then one fp32 rounding of a value of at most 1 (2^-24) and the fp64 steps (1e-12)."""
    nm, nd = np.sqrt((m * m).sum(-1, keepdims=True)), np.sqrt((delta * delta).sum(-1, keepdims=True))
    low = nm - nd
    with np.errstate(divide="ignore", invalid="ignore"):
        bar = delta / low + np.abs(m) * nd / (low * nm) + 2.0 ** -24 + 1e-12
    return np.where(low > 0.0, bar, np.inf)


def ranges_of(N, K):
    """the update's point ranges: (R, L) = (min(ceil(N / 256), 4096 // K clamped to 16 .. 64), ceil(N / R))"""
    R = min(min(MAX_RANGES, max(MIN_RANGES, RANGE_WGS // K)), -(-N // RANGE_MIN))
    return R, -(-N // R)


def scratch_bytes(B, n, K, D):
    N = B * n
    return 4 * ranges_of(N, K)[0] * K * (D + 1) + 8 * (-(-N // 64))


def scratch_sums(scratch_u8, N, K, D):
    """the device's m_j as the finalize launch forms it: the scratch's partial sums fp32 [R][K][D] added in range order in fp32, and
    the partial counts int32 [R][K] added; scratch as a uint8 numpy array"""
    R, _ = ranges_of(N, K)
    psum = scratch_u8[:4 * R * K * D].view(np.float32).reshape(R, K, D)
    pcount = scratch_u8[4 * R * K * D:4 * R * K * (D + 1)].view(np.int32).reshape(R, K)
    m = np.zeros((K, D), dtype=np.float32)
    for r in range(R):
        m = m + psum[r]
    return m, pcount.sum(axis=0).astype(np.int64)


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------
def normal_tokens(seed, B, n, D):
    """unnormalised Gaussian rows with a CLS row in front: fp32 [B, 1 + n, D]"""
    return np.random.default_rng(seed).standard_normal((B, n + 1, D)).astype(np.float32)


def planted_tokens(seed, B, n, D, K, noise=0.5, scale=3.0):
    """K planted unit directions, every cell = scale (its direction + noise x a unit noise row): (tokens fp32 [B, 1 + n, D] with a CLS
    row in front, planted labels int64 [B n])"""
    rng = np.random.default_rng(seed)
    dirs = unit_rows(rng.standard_normal((K, D)))
    lab = rng.integers(0, K, B * n)
    lab[:min(K, B * n)] = np.arange(K)[:min(K, B * n)]                  # every cluster is planted at least once where N allows
    x = dirs[lab] + noise * unit_rows(rng.standard_normal((B * n, D)))
    tok = np.zeros((B, n + 1, D), dtype=np.float32)
    tok[:, 1:] = (scale * x).reshape(B, n, D).astype(np.float32)
    tok[:, 0] = rng.standard_normal((B, D)).astype(np.float32)
    return tok, lab.astype(np.int64)
