"""The normalized-cut rule of include/dinoseg.h (dinoseg_op_ncut_graph and dinoseg_op_ncut_iterate) restated in int64 / fp64 numpy:
the scores and the bit graph of a frame, its packing into uint64 words, the weights r and u, the deflate-and-normalise step, one
lazy pass, the result rule, the plain matrix form of the same iteration, and the error bars of the device's fp32 steps."""
import numpy as np

EPS32 = 2.0 ** -24              # half an ulp of an fp32 value of magnitude 1: the relative error of one fp32 rounding


def score_bar(D):
    """E(D) = (D + 16) 2^-24, the bar of the three-product fp16 MFMA score (tests/kmeans_util.py: score_bar)"""
    return (D + 16) * 2.0 ** -24


def frame_points(planes):
    """point planes fp16 [B, 2, n, D] (hi, lo; scaled by 2^10) -> the rows they DEFINE, fp64 [B, n, D] = (hi + lo) 2^-10"""
    p = np.asarray(planes).astype(np.float64)
    return (p[:, 0] + p[:, 1]) * 2.0 ** -10


def scores_host(X):
    """X fp64 [n, D] -> S fp64 [n, n] = <x_i, x_j>, -0 taken as +0"""
    return X @ X.T + 0.0


def words_of(n):
    return -(-n // 64)


def pack_bits(bits):
    """bool [n, n] -> uint64 [n, ceil(n / 64)]: key j at bit j % 64 of word j // 64, pad bits zero"""
    n, W = bits.shape[0], words_of(bits.shape[1])
    padded = np.zeros((n, W * 64), dtype=np.uint8)
    padded[:, :bits.shape[1]] = bits
    return np.packbits(padded.reshape(n, W, 64), axis=2, bitorder="little").reshape(n, W, 8).copy().view("<u8").reshape(n, W)


def unpack_words(words, n):
    """uint64 [rows, W] -> (bool [rows, n], bool [rows, 64 W - n] the pad bits)"""
    w = np.ascontiguousarray(words).astype("<u8")
    b = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little").astype(bool)
    return b[:, :n], b[:, n:]


def weights(cnt, n, eps):
    """cnt int64 [n] -> (d, r, u) as fp64 arrays holding the rule's fp32 values: d_i = fp32(eps (n - cnt_i) + cnt_i),
    r_i = fp32(1 / sqrt(d_i)) (0 where d_i = 0), u_i = fp32(sqrt(d_i) / sqrt(sum d)) (0 where the sum is 0)"""
    cnt = np.asarray(cnt, dtype=np.float64)
    d = (eps * (n - cnt) + cnt).astype(np.float32).astype(np.float64)
    with np.errstate(divide="ignore"):
        r = np.where(d > 0.0, 1.0 / np.sqrt(d), 0.0).astype(np.float32).astype(np.float64)
    tot = np.sqrt(d.sum())
    u = (np.sqrt(d) / tot if tot > 0.0 else np.zeros_like(d)).astype(np.float32).astype(np.float64)
    return d, r, u


def dn(z, u):
    """deflate and normalise in fp64: q = z - <u, z> u, z' = q / ||q|| (0 where ||q|| = 0) -> (z', q, ||q||)"""
    z = np.asarray(z, dtype=np.float64)
    q = z - (u @ z) * u
    nrm = np.sqrt(q @ q)
    return (q / nrm if nrm > 0.0 else np.zeros_like(q)), q, nrm


def one_pass(bits_f, r, u, eps, z_in):
    """One call with iters = 1 in fp64 from the caller's vector: z0 = DN(z_in), the pass, z' = DN(p).  bits_f: the graph as fp64
    [n, n].  -> dict(z0, c0 = <u, z_in>, n0 = the first norm, xv, A = sum over set bits of |xv_j|, S, t, y, rho, p, c = <u, p>, q, nrm, z)"""
    z0, _, n0 = dn(z_in, u)
    xv = z0 * r
    t = bits_f @ xv
    A = bits_f @ np.abs(xv)
    S = xv.sum()
    y = r * (eps * S + (1.0 - eps) * t)
    rho = z0 @ y
    p = 0.5 * (z0 + y)
    z, q, nrm = dn(p, u)
    return dict(z0=z0, c0=float(u @ np.asarray(z_in, dtype=np.float64)), n0=n0, xv=xv, A=A, S=S, t=t, y=y, rho=rho, p=p, c=float(u @ p),
                q=q, nrm=nrm, z=z)


def iterate_host(bits_f, r, u, eps, start, iters):
    """the call in fp64: (z after iters passes (prepared: DN of the last p, or of the start for iters = 0), rho [iters])"""
    z, rho = np.asarray(start, dtype=np.float64), []
    for _ in range(iters):
        o = one_pass(bits_f, r, u, eps, z)
        z = o["z"]
        rho.append(o["rho"])
    return dn(z, u)[0], np.array(rho)


def result_host(z, r):
    """step 7 in fp64 on a prepared z -> dict(v, avg, seed, sigma, margin, fg, eigvec)"""
    v = z * r
    avg = v.mean()
    seed = int(np.argmax(np.abs(v)))                                    # (numpy returns the first maximum)
    sigma = 1.0 if v[seed] > avg else -1.0
    margin = sigma * (v - avg)
    return dict(v=v, avg=avg, seed=seed, sigma=sigma, margin=margin, fg=margin > 0.0, eigvec=sigma * v)


def matrix_form(bits_f, r, u, eps, start, iters):
    """The plain matrix form: dense W = eps 11^T + (1 - eps) Bits, M = diag(r) W diag(r), the lazy deflated iteration on (I + M) / 2 with
    explicit matrices -> (z, rho [iters], M)"""
    n = bits_f.shape[0]
    Wm = eps * np.ones((n, n)) + (1.0 - eps) * bits_f
    M = r[:, None] * Wm * r[None, :]
    L = 0.5 * (np.eye(n) + M)
    P = np.eye(n) - np.outer(u, u)

    def prep(z):
        q = P @ z
        nrm = np.linalg.norm(q)
        return q / nrm if nrm > 0.0 else np.zeros(n)

    z, rho = prep(np.asarray(start, dtype=np.float64)), []
    for _ in range(iters):
        rho.append(z @ M @ z)
        z = prep(prep(L @ z))                                           # (the next pass prepares its input once more)
    return z, np.array(rho), M


def pass_bars(o, bits_f, cnt, r, u, eps):
    """The bars of one device call with iters = 1 against `o = one_pass(...)` on the same graph and z_in, from the operation counts
    (e = 2^-24, one fp32 rounding of a value x costs e |x|; r_i and u_i are themselves fp32 roundings of fp64 expressions, and the
    device's may fall on the other side of a tie: one more e on every product with them):
      z0 = DN(z_in): two elementwise roundings (q, the quotient), a norm that moves by at most e relative, and u's own rounding in
           c0 u_i: dz0_i = 4 e |z0_i| + 2 e |c0| u_i / N0;
      xv_i = fp32(z0_i r_i): dxv_i = r_i dz0_i + 2 e |xv_i|;
      t_i: an fp32 sum of cnt_i terms in any order, (cnt_i + 16) e A_i with A_i = the sum over the set bits of |xv_j|, and the terms'
           own errors: dt_i = (cnt_i + 16) e A_i + sum over the set bits of dxv_j;
      S (fp64): dS = sum_j dxv_j;
      y_i = fp32(r_i (eps S + (1 - eps) t_i)): dy_i = r_i (eps dS + (1 - eps) dt_i) + 2 e |y_i|;
      rho = fp32(<z0, y>): drho = sum_i (|z0_i| dy_i + dz0_i |y_i|) + e |rho|;
      p_i = fp32((z0_i + y_i) / 2): dp_i = (dz0_i + dy_i) / 2 + e |p_i|;
      c = <u, p>: dc = sum_i u_i dp_i + e sum_i u_i |p_i|;  q_i = fp32(p_i - c u_i): dq_i = dp_i + (dc + e |c|) u_i + e |q_i|;
      z'_i = fp32(q_i / ||q||): dz_i = dq_i / N' + |q_i| ||dq|| / (N N') + e |z'_i|, N = ||q||, N' = N - ||dq|| (inf where N' <= 0);
    every bar gets 1e-12 for the fp64 steps.  `bits_f` is the graph as fp64 [n, n].  -> (dz [n], drho, dt [n])"""
    e = EPS32
    dz0 = 4.0 * e * np.abs(o["z0"]) + (2.0 * e * abs(o["c0"]) * u / o["n0"] if o["n0"] > 0.0 else 0.0)
    dxv = r * dz0 + 2.0 * e * np.abs(o["xv"])
    dt = (cnt + 16.0) * e * o["A"] + bits_f @ dxv
    dS = dxv.sum()
    dy = r * (eps * dS + (1.0 - eps) * dt) + 2.0 * e * np.abs(o["y"])
    drho = float((np.abs(o["z0"]) * dy + dz0 * np.abs(o["y"])).sum() + e * abs(o["rho"])) + 1e-12
    dp = 0.5 * (dz0 + dy) + e * np.abs(o["p"])
    dc = float(u @ dp) + e * float(u @ np.abs(o["p"]))
    dq = dp + (dc + e * abs(o["c"])) * u + e * np.abs(o["q"])
    N, nd = o["nrm"], float(np.sqrt(dq @ dq))
    if N - nd > 0.0:
        dz = dq / (N - nd) + np.abs(o["q"]) * nd / (N * (N - nd)) + e * np.abs(o["z"]) + 1e-12
    else:
        dz = np.full_like(dq, np.inf)
    return dz, drho, dt


def result_bars(res):
    """Step 7 on the device's own z: v_i = fp32(z_i r_i) is one rounding of the product, and r_i may be the other neighbour of its tie:
    dv_i = 2 e |v_i|; the fp64 mean of such values moves by at most 2 e mean|v|: davg.  -> (dv [n], davg)"""
    return 2.0 * EPS32 * np.abs(res["v"]) + 1e-30, 2.0 * EPS32 * float(np.abs(res["v"]).mean()) + 1e-30


# ---- seeded inputs -------------------------------------------------------------------------------------------------------------
def unit_rows(rows):
    r = np.asarray(rows, dtype=np.float64)
    return r / np.maximum(np.sqrt((r * r).sum(-1, keepdims=True)), 1e-12)


def normal_tokens(seed, B, n, D):
    """unnormalised Gaussian rows with a CLS row in front: fp32 [B, 1 + n, D]"""
    return np.random.default_rng(seed).standard_normal((B, n + 1, D)).astype(np.float32)


def planted_tokens(seed, B, n, D, noise=0.5, scale=3.0):
    """Two planted orthogonal unit directions per frame, every cell = scale (its direction + noise x a unit noise row); the first third of a
    shuffled order (at least one cell where n >= 2) takes direction 0: (tokens fp32 [B, 1 + n, D] with a CLS row in front, small bool
    [B, n]: the cells of the smaller group)"""
    rng = np.random.default_rng(seed)
    tok = np.zeros((B, n + 1, D), dtype=np.float32)
    small = np.zeros((B, n), dtype=bool)
    for b in range(B):
        dirs = unit_rows(rng.standard_normal((2, D)))
        dirs[1] = unit_rows(dirs[1] - (dirs[1] @ dirs[0]) * dirs[0])     # orthogonal: the cosine across the groups is noise alone
        k = max(n // 3, 1) if n >= 2 else 0
        small[b, rng.permutation(n)[:k]] = True
        lab = np.where(small[b], 0, 1)
        x = dirs[lab] + noise * unit_rows(rng.standard_normal((n, D)))
        tok[b, 1:] = (scale * x).astype(np.float32)
        tok[b, 0] = rng.standard_normal(D).astype(np.float32)
    return tok, small
