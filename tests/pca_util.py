"""Shared by tests/test_pca_cpu.py and tests/test_pca_gpu.py: the rules of include/dinoseg.h's PCA section restated in numpy -- the
point c = fp32(x - shift), its fp64 sums, the bars computed from the same c, the range rule R(B n, D), the scratch size, the projection
and the colour rule in int64 coordinates / fp64 -- and the operator cases."""
import numpy as np

U = 2.0 ** -24

# (B, n, D, keep): keep is None, "random" or "random0" (random with frame 1 all zero)
MOMENT_CASES = [
    (1, 1, 64, None),               # one row
    (1, 2, 64, None),               # one MFMA k-pair
    (1, 3, 64, None),               # an odd row count
    (2, 35, 64, "random"),          # the CLS skip across frames
    (1, 65, 192, None),
    (3, 480, 384, "random0"),       # one frame all zero
    (1, 1200, 1024, None),          # the widest
    (2, 4800, 384, "random"),       # the camera grid, several ranges
]
# (B, n, D, q)
PROJECT_CASES = [(1, 1, 64, 1), (1, 5, 64, 3), (2, 35, 192, 33), (1, 65, 384, 64), (2, 480, 384, 128), (1, 192, 1024, 256),
                 (1, 4800, 384, 3)]
# (hp, wp, OH, OW, q)
COLOUR_CASES = [(1, 1, 1, 1, 3), (1, 1, 8, 8, 3), (3, 4, 24, 32, 3), (5, 7, 37, 53, 5), (60, 80, 480, 640, 3)]


def case_id(c):
    return "-".join(str(v) for v in c)


# ---- the range rule and the scratch
def pairs(D):
    T = D // 64
    return T * (T + 1) // 2


def ranges(N, D):
    """R(B n, D) = max(1, min(64, ceil(N / 128), ceil(2048 / P)))"""
    return max(1, min(64, -(-N // 128), -(-2048 // pairs(D))))


def range_len(N, D):
    return -(-N // ranges(N, D))


def scratch_bytes(B, n, D):
    if B < 1 or n < 1 or B * n > 2 ** 31 - 256 or D < 64 or D > 1024 or D % 64:
        return -1
    return 4 * ranges(B * n, D) * (4096 * pairs(D) + D + 1)


# ---- the moments
def make_tokens(B, n, D, seed, offset=2.0):
    """fp32 [B, 1 + n, D]: unit noise around a common mean of `offset` per column sign pattern, as final-norm features have; the CLS
    rows are large, so that a counted CLS row shows"""
    rng = np.random.default_rng(seed)
    mean = offset * rng.choice([-1.0, 1.0], D) * rng.random(D)
    x = (rng.standard_normal((B, 1 + n, D)) + mean).astype(np.float32)
    x[:, 0, :] = 1.0e3
    return x


def make_keep(B, n, kind, seed):
    if kind is None:
        return None
    keep = (np.random.default_rng(seed).random((B, n)) < 0.7).astype(np.uint8)
    if kind == "random0" and B > 1:
        keep[1] = 0
    return keep


def points(tokens, keep, shift):
    """the rule's points: c = fp32(x - shift), one fp32 subtraction; rows not kept are zeros.  fp32 [B n, D] and the kept flags"""
    B, n1, D = tokens.shape
    sh = np.zeros(D, np.float32) if shift is None else np.asarray(shift, np.float32)
    c = (tokens[:, 1:, :].astype(np.float32) - sh[None, None, :]).astype(np.float32).reshape(B * (n1 - 1), D)
    kept = np.ones(c.shape[0], bool) if keep is None else np.asarray(keep).reshape(-1) != 0
    c[~kept] = 0.0
    return c, kept


def moments(c, kept):
    """(sum fp64 [D], outer fp64 [D, D], count) of the points, in fp64"""
    c64 = c.astype(np.float64)
    return c64.sum(axis=0), c64.T @ c64, int(kept.sum())


def moment_bars(c, L):
    """(bar of sum [D], bar of outer [D, D]): (L + 16) 2^-24 sum |c[d]| and (L + 16) 2^-24 sum |c[d] c[e]|"""
    a = np.abs(c.astype(np.float64))
    return (L + 16) * U * a.sum(axis=0), (L + 16) * U * (a.T @ a)


# ---- the projection
def project(tokens, mean, basis, scale=None):
    """(y fp64 [B, n, q], bar [B, n, q]) of c = fp32(x - mean) in fp64: y = c basis^T (times scale), bar = (D + 16) 2^-24 |c| |basis|^T
    (times |scale|)"""
    D = tokens.shape[2]
    c = (tokens[:, 1:, :].astype(np.float32) - np.asarray(mean, np.float32)[None, None, :]).astype(np.float32).astype(np.float64)
    b = np.asarray(basis, np.float64)
    y, bar = c @ b.T, (D + 16) * U * (np.abs(c) @ np.abs(b).T)
    if scale is not None:
        s = np.asarray(scale, np.float64)
        y, bar = y * s, bar * np.abs(s)
    return y, bar


# ---- the colour rule
def axis_coords(i, o):
    """the integer coordinates of dinoseg_op_upsample_argmax along one axis (input i, output o): (i0, i1, lambda) with lambda in fp64"""
    d = np.arange(o, dtype=np.int64)
    num = np.maximum((2 * d + 1) * i - o, 0)
    den = 2 * o
    q, rem = num // den, num % den
    last = q >= i - 1
    q = np.where(last, i - 1, q)
    rem = np.where(last, 0, rem)
    return q, np.minimum(q + 1, i - 1), rem.astype(np.float64) / den


def colour(comps, hp, wp, lo, inv, keep, OH, OW):
    """comps fp32 [B, 1 + hp wp, q] -> (255 t clamped, fp64 [B, OH, OW, 3]; kept pixels bool [B, OH, OW]; max |t| over the cells)"""
    B = comps.shape[0]
    t = (comps[:, 1:, :3].astype(np.float64) - np.asarray(lo, np.float64)) * np.asarray(inv, np.float64)
    t = t.reshape(B, hp, wp, 3)
    x0, x1, lx = axis_coords(wp, OW)
    y0, y1, ly = axis_coords(hp, OH)
    h = t[:, :, x0, :] + (t[:, :, x1, :] - t[:, :, x0, :]) * lx[None, None, :, None]
    v = h[:, y0] + (h[:, y1] - h[:, y0]) * ly[None, :, None, None]
    cy, cx = (np.arange(OH, dtype=np.int64) * hp) // OH, (np.arange(OW, dtype=np.int64) * wp) // OW
    kept = np.ones((B, OH, OW), bool) if keep is None else (np.asarray(keep).reshape(B, hp, wp) != 0)[:, cy][:, :, cx]
    return 255.0 * np.clip(v, 0.0, 1.0), kept, float(np.abs(t).max()), v


def colour_bar(tmax):
    """in bytes: 255 (16 max|t| + 1) 2^-24.  Per lerp a + (b - a) lambda with values of either sign, |v| <= M: the difference's rounding
    is at most 2 M u, lambda's (one correctly rounded quotient) moves the product by at most 2 M u, the fused multiply-add rounds once,
    M u: 5 M u, and two chained lerps 10 M u; t itself is one subtraction and one multiplication in fp32 against fp64, 2 M u; 16 leaves
    room for the second-order terms.  The clamp does not grow an error, and 255 t is one more rounding of a value <= 255: 255 u."""
    return 255.0 * (16.0 * tmax + 1.0) * U
