"""Exact probes of the split-plane pair walk (dino_amd/csrc/pair_common.h) and of its three consumers, kmeans_assign_kernel,
ncut_graph_kernel and propagate_scores_kernel: the builders of the inputs, the int64 / fp64 references, and an fp32 emulation of
the walk with mutants.  Nothing here launches a kernel.

Every operator takes its fp16 hi + lo planes as input, so a test may hand it ANY fp16 values, not only the split of a unit row.
The probes hand it planes whose entries are m 2^e with small integers m, the hi and the lo plane drawn INDEPENDENTLY of each other
(lo is not the remainder of anything).  Then

    S = hi_q . hi_k + hi_q . lo_k + lo_q . hi_k                                        (an integer; lo . lo is NOT part of it)

and what a kernel holds is S 2^(2e) in its fp32 accumulators and s = S 2^(2e - 20) after the unscale.  EXACTNESS CONDITION: every
MFMA adds products of two plane entries, |product| <= max|m|^2 2^(2e), and an accumulator never holds more than the 3 D products of
one pair, so with 3 D max|m|^2 < 2^24 every partial sum, in ANY order of summation and with one accumulator or three, is an integer
multiple of 2^(2e) below 2^(24 + 2e): exact in fp32.  The multiplication by 2^-20 is exact, "+ 0.f" turns -0 into +0 (the reference:
an int64 zero times the scale is +0.0).  The reference is then the only right answer bit for bit: no band, no undecided cases.  The
independent lo planes give each of the three terms full weight and make lo . lo as large as any of them, so a kernel that adds it,
drops a term, or reads one 8-half chunk from the wrong place is off by whole integers.

What these probes cannot see: the arithmetic of normalize_tokens and split_unit (the planes are inputs here); the fp64 tests of the
three operators cover it."""
import types

import numpy as np

from tests import kmeans_util as KM
from tests import propagate_util as P

TILE = 64                                # query rows of a workgroup, key rows of a block, halves of a slice (PAIR_TILE)
U = 2.0 ** -24                           # unit roundoff of fp32 (tests/probe_util.py)
ULP = 2.0 * U                            # one ulp relative to the value, at worst: the error taken for v_exp_f32
INT_MAX = 2 ** 31 - 1


# ---- integer planes ------------------------------------------------------------------------------------------------------------
def exact_ok(D, mmax):
    """the exactness condition of the module's docstring"""
    return 3 * D * mmax * mmax < 2 ** 24


def scale(e):
    """what one unit of the integer score S is worth in the kernel's output: 2^(2e - 20)"""
    return 2.0 ** (2 * e - 20)


def draw(rng, shape, mmax, density):
    """int64 entries in [-mmax, mmax], zero with probability 1 - density (and where the integer drawn is zero)"""
    m = rng.integers(-mmax, mmax + 1, size=shape)
    return np.where(rng.random(shape) < density, m, 0).astype(np.int64)


def int_planes(seed, shape, mmax, density):
    """(hi, lo) int64 of `shape` (..., rows, D), two independent draws"""
    rng = np.random.default_rng(seed)
    return draw(rng, shape, mmax, density), draw(rng, shape, mmax, density)


def to_f16(m, e):
    v = (np.asarray(m, dtype=np.float64) * 2.0 ** e).astype(np.float16)
    assert np.array_equal(v.astype(np.float64), np.asarray(m, dtype=np.float64) * 2.0 ** e), "m 2^e is not an fp16 value"
    return v


def stack_planes(hi, lo, e):
    """int64 [..., rows, D] twice -> fp16 [..., 2, rows, D], the layout of every operator"""
    return np.ascontiguousarray(np.stack([to_f16(hi, e), to_f16(lo, e)], axis=-3))


def int_scores(qh, ql, kh, kl):
    """S int64 [nq, nk]: the three terms, without lo . lo"""
    return qh @ kh.T + qh @ kl.T + ql @ kh.T


def f32_of(S, e):
    """the fp32 the kernel must hold for the integer S: S 2^(2e - 20), exactly (|S| < 2^24), -0 never"""
    assert np.abs(S).max(initial=0) < 2 ** 24
    v = (np.asarray(S, dtype=np.float64) * scale(e)).astype(np.float32)
    assert np.array_equal(v.astype(np.float64), np.asarray(S, dtype=np.float64) * scale(e))
    return v + np.float32(0.0)


def rank_rows(s, g):
    """rows of candidates in the total order of better(): score descending, index ascending"""
    order = np.lexsort((g, -s), axis=-1)
    return np.take_along_axis(s, order, axis=1), np.take_along_axis(g, order, axis=1)


# ---- kmeans --------------------------------------------------------------------------------------------------------------------
# (B, n, D, K); then (max|m|, density, e) and the centroids that are copies of earlier ones: (copy, of)
KM_CASES = [(1, 77, 64, 5), (2, 100, 192, 65), (1, 130, 384, 64), (1, 70, 768, 256)]
KM_DRAW = [(1, 0.5, 0), (2, 0.3, 3), (8, 0.5, -2), (1, 0.25, 6)]
KM_COPIES = [((4, 0), (2, 1)), ((64, 4), (32, 1), (40, 3)), ((63, 0), (36, 33)), ((255, 4), (128, 68), (70, 65))]
# the update: (1, 1100, 64, 3) (5 ranges of 220 points: ranges_of) and one whose 64 ranges hold 1032 points each,
# more than one list of 1024
KM_UPDATE_CASES = [(1, 1100, 64, 3), (1, 66048, 64, 3)]


def kmeans_case(i):
    """dict(points (hi, lo) int64 [B, n, D], cent (hi, lo) int64 [K, D], e, mmax).  Some centroids are exact copies of earlier ones
    (KM_COPIES): every point ties between the two, across lanes, waves and blocks, on top of the ties small integers give anyway."""
    B, n, D, K = KM_CASES[i]
    mmax, density, e = KM_DRAW[i]
    assert exact_ok(D, mmax)
    ph, pl = int_planes(7100 + i, (B, n, D), mmax, density)
    ch, cl = int_planes(7200 + i, (K, D), mmax, density)
    for dst, src in KM_COPIES[i]:
        ch[dst], cl[dst] = ch[src], cl[src]
    return dict(points=(ph, pl), cent=(ch, cl), e=e, mmax=mmax, shape=KM_CASES[i])


def kmeans_ref(case):
    """dict(S int64 [N, K], scores fp32 [N, K], assign int64 [N] (the first maximum), best fp32 [N], prev int32 [N], moved int,
    objective fp32, obj_abs: sum |S_best|, which must stay below 2^24 for the objective's fp32 sums to be exact in any order)"""
    B, n, D, K = case["shape"]
    ph, pl = (p.reshape(B * n, D) for p in case["points"])
    ch, cl = case["cent"]
    S = int_scores(ph, pl, ch, cl)
    a = np.argmax(S, axis=1)                                            # (numpy returns the first maximum)
    best = S[np.arange(B * n), a]
    prev = a.copy()
    rng = np.random.default_rng(7300 + K)
    flip = rng.random(B * n) < 0.3
    prev[flip] = rng.integers(0, K, size=int(flip.sum()))
    return dict(S=S, scores=f32_of(S, case["e"]), assign=a.astype(np.int64), best=f32_of(best, case["e"]), prev=prev.astype(np.int32),
                moved=int((prev != a).sum()), objective=f32_of(np.array([best.sum()]), case["e"])[0], obj_abs=int(np.abs(best).sum()))


def kmeans_update_case(i):
    """dict(points (hi, lo) int64 [B, n, D], assign int32 [N], e, R, L, psum fp32 [R, K, D] exact, pcount int64 [R, K], sum_abs)"""
    B, n, D, K = KM_UPDATE_CASES[i]
    e, mmax = 2, 8
    ph, pl = int_planes(7400 + i, (B, n, D), mmax, 0.7)
    N = B * n
    a = np.random.default_rng(7500 + i).integers(0, K, size=N).astype(np.int32)
    R, L = KM.ranges_of(N, K)
    x = (ph + pl).reshape(N, D)                                         # x = (hi + lo) 2^-10: the integer (m_hi + m_lo) times 2^(e - 10)
    psum, pcount, worst = np.zeros((R, K, D), dtype=np.int64), np.zeros((R, K), dtype=np.int64), 0
    for r in range(R):
        lo_i, hi_i = min(r * L, N), min(r * L + L, N)
        for j in range(K):
            members = x[lo_i:hi_i][a[lo_i:hi_i] == j]
            psum[r, j], pcount[r, j] = members.sum(axis=0), members.shape[0]
            worst = max(worst, int(np.abs(members).sum(axis=0).max(initial=0)))
    return dict(points=(ph, pl), assign=a, e=e, R=R, L=L, psum=(psum.astype(np.float64) * 2.0 ** (e - 10)).astype(np.float32),
                pcount=pcount, sum_abs=worst, shape=KM_UPDATE_CASES[i])


# ---- the 1-bit graph: the threshold sweep ----------------------------------------------------------------------------------------
# (B, hp, wp, D); ternary planes of density p with 3 D p^2 near 50, so that the off-diagonal scores spread over
# about +-30 and the sweep needs fewer than 128 launches; e per case
NC_CASES = [(1, 5, 13, 64), (2, 9, 11, 192), (1, 10, 13, 384), (1, 7, 10, 768)]
NC_DRAW = [(0.5, 0), (0.29, 2), (0.2, 4), (0.145, -1)]
MAX_SWEEP = 128


def ncut_case(i):
    B, hp, wp, D = NC_CASES[i]
    density, e = NC_DRAW[i]
    assert exact_ok(D, 1)
    hi, lo = int_planes(7600 + i, (B, hp * wp, D), 1, density)
    return dict(planes=(hi, lo), e=e, shape=NC_CASES[i])


def ncut_ref(case):
    """dict(S int64 [B, n, n], t0, t1: the window of thresholds, one step wider on either side than the off-diagonal scores, so an
    off-diagonal pair's count S - t0 lies in 1 .. t1 - t0 and a score wrong in either direction moves it; counts int64 [B, n, n] =
    clamp(S, t0, t1 + 1) - t0, the number of thresholds tau_t = (t + 1/2) 2^(2e - 20), t0 <= t <= t1, that the pair's score exceeds)"""
    hi, lo = case["planes"]
    S = np.stack([int_scores(hi[b], lo[b], hi[b], lo[b]) for b in range(hi.shape[0])])
    n = S.shape[1]
    off = S[:, ~np.eye(n, dtype=bool)]
    t0, t1 = int(off.min()) - 1, int(off.max())
    return dict(S=S, t0=t0, t1=t1, counts=np.clip(S, t0, t1 + 1) - t0)


def sweep_taus(t0, t1, e):
    """the half-integer thresholds of the window as Python floats, each exact in fp32 and inside (-1, 1)"""
    taus = [(t + 0.5) * scale(e) for t in range(t0, t1 + 1)]
    for tau in taus:
        assert float(np.float32(tau)) == tau and -1.0 < tau < 1.0
    return taus


# ---- the 1-bit graph: indicator frames -------------------------------------------------------------------------------------------
IND_V = 32.0                             # the one non-zero value of an indicator plane: every product is 2^10, the threshold 2^9
IND_TAU = 0.5 * IND_V * IND_V * 2.0 ** -20


def indicator_phases(n, D):
    """launched frames needed: a phase gives the hi . hi term floor(n / 2) columns of its own and the cross terms one fewer"""
    return -(-D // (n // 2 - 1))


def indicator_maps(n, D, phase):
    """(u, w) int64 [n]: row i has hi = one-hot at u(i), lo = one-hot at w(i) != u(i).  Logical rows 2m and 2m + 1 share u = base + m;
    w = u + 1 for the even and u + 2 for the odd one (mod D), so that
      rows 2m, 2m + 1               meet in hi . hi alone at column base + m,
      row 2m and the rows of m + 1  meet in hi . lo / lo . hi alone at column base + m + 1,
      row 2m + 1 and row 2m + 2     meet in lo . lo alone (w = base + m + 2 for both): their bit is 0.
    A seeded permutation spreads the logical rows over the frame, so the meeting pairs lie in any two tiles and key blocks."""
    step = n // 2 - 1
    logical = np.random.default_rng(7700 + 31 * phase + n).permutation(n)
    m, odd = logical // 2, logical % 2
    u = (phase * step + m) % D
    return u.astype(np.int64), ((u + 1 + odd) % D).astype(np.int64)


def indicator_planes(u, w, D):
    """fp16 [2, n, D]"""
    n = u.shape[0]
    p = np.zeros((2, n, D), dtype=np.float16)
    p[0, np.arange(n), u] = IND_V
    p[1, np.arange(n), w] = IND_V
    return p


def indicator_terms(u, w):
    """bool [n, n] each: hh = [u_i = u_j], hl = [u_i = w_j], lh = [w_i = u_j], ll = [w_i = w_j]; the bit is hh | hl | lh"""
    return u[:, None] == u[None, :], u[:, None] == w[None, :], w[:, None] == u[None, :], w[:, None] == w[None, :]


def indicator_coverage(n, D):
    """(columns that the hi . hi, hi . lo and lo . hi term decide ALONE at an off-diagonal pair, each a set; the number of off-diagonal
    pairs that meet in lo . lo alone) over all phases"""
    cols, only_ll = [set(), set(), set()], 0
    offd = ~np.eye(n, dtype=bool)
    for phase in range(indicator_phases(n, D)):
        u, w = indicator_maps(n, D, phase)
        assert np.all(u != w)
        hh, hl, lh, ll = indicator_terms(u, w)
        col_of = (np.broadcast_to(u[:, None], (n, n)), np.broadcast_to(u[:, None], (n, n)), np.broadcast_to(w[:, None], (n, n)))
        for t, (own, a, b) in enumerate(((hh, hl, lh), (hl, hh, lh), (lh, hh, hl))):
            cols[t] |= set(col_of[t][own & ~a & ~b & offd].tolist())
        only_ll += int((ll & ~hh & ~hl & ~lh & offd).sum())
    return cols, only_ll


# ---- propagate -------------------------------------------------------------------------------------------------------------------
# (hp, wp, D, C, n_ctx, R, k), the last with a single candidate per context frame for k = 5 (the first four
# never run out of candidates); (max|m|, density).  e = 8 for all: s = S / 16, so with tau = 0.1 a score one integer below the best
# has (s - s0) / tau = -0.625 and the weights are not all 1
PR_CASES = [(5, 7, 64, 3, 1, 2, 5), (9, 11, 64, 7, 2, 12, 5), (12, 16, 384, 5, 3, 3, 5), (9, 11, 768, 4, 2, 12, 1), (3, 4, 64, 2, 2, 0, 5)]
PR_DRAW = [(1, 0.4), (2, 0.25), (1, 0.2), (1, 0.15), (1, 0.5)]
PR_E = 8
PR_TAU = 0.1


def prop_case(i):
    hp, wp, D, C, n_ctx, R, k = PR_CASES[i]
    mmax, density = PR_DRAW[i]
    assert exact_ok(D, mmax)
    n = hp * wp
    th, tl = int_planes(7800 + i, (n, D), mmax, density)
    kh, kl = int_planes(7900 + i, (n_ctx, n, D), mmax, density)
    segs = np.random.default_rng(8000 + i).random((n_ctx, n, C)).astype(np.float32)
    return dict(target=(th, tl), ctx=(kh, kl), segs=segs, e=PR_E, shape=PR_CASES[i])


def prop_ref(case, tau=PR_TAU):
    """dict(g int64 [n, k] in rank order, -1 beyond the candidates; s fp64 [n, k] the exact scores (-inf beyond); count int64 [n];
    wn fp64 [n, k] and V fp64 [n, C] formed in fp64 from the exact scores with the kernel's a = fp32(log2 e / tau); bar_w [n, k] and
    bar_v [n, C]; x_min: the most negative (s - s0) / tau of a selected candidate).

    The bars, from propagate_merge_kernel's instruction sequence.  d = s - s0 is exact (both are integers times 2^(2e - 20), below
    2^24 of them).  x = fl(d a): one rounding, |dx| <= |x| U.  w = v_exp_f32(x): 2^x (1 + |x| U ln 2 + ..) within one ulp (ULP,
    taken as in tests/probe_util.py), and a result below 2^-126 may be flushed: an absolute 2^-126.  W = the sum of k such terms in
    fp32: k - 1 additions, each U.  inv = 1 / W correctly rounded: U.  topk_w = fl(w inv): U.  With dw = xmax U ln 2 + ULP (xmax: the
    largest |x| of the query) the relative error of w inv is at most rw = 2 dw + (k + 1) U to first order, rw / (1 - rw) in all;
    w / W <= 1.  seg_out = fl(v inv) with v a chain of k fused multiply-adds: each rounds the running sum once, k U relative to
    sum_i w_i |seg_i|, and carries the w's dw; times inv (dw + (k - 1) U + U) and the product's U: rv = 2 dw + (2 k + 1) U relative to
    A = sum_i (w_i / W) |seg_i|.  The flush adds at most k 2^-126 max|seg| (W >= 1: w_0 = 1).  No E term: the scores are exact."""
    hp, wp, D, C, n_ctx, R, k = case["shape"]
    n = hp * wp
    th, tl = case["target"]
    kh, kl = case["ctx"]
    idx, valid = P.neighbours(hp, wp, R)
    s_all, g_all = [], []
    for ci in range(n_ctx):
        S = int_scores(th, tl, kh[ci], kl[ci]).astype(np.float64) * scale(case["e"])
        s_all.append(np.where(valid, np.take_along_axis(S, idx, axis=1), -np.inf))
        g_all.append(np.where(valid, ci * n + idx, np.iinfo(np.int64).max))
    s, g = rank_rows(np.concatenate(s_all, axis=1) + 0.0, np.concatenate(g_all, axis=1))
    count = np.isfinite(s).sum(axis=1)
    kk = min(k, s.shape[1])
    s_sel, g_sel = np.full((n, k), -np.inf), np.full((n, k), -1, dtype=np.int64)
    s_sel[:, :kk], g_sel[:, :kk] = s[:, :kk], np.where(np.isfinite(s[:, :kk]), g[:, :kk], -1)
    wn, V = P.weights_and_value(s_sel, g_sel, case["segs"], tau)
    ok = g_sel >= 0
    x = np.where(ok, (np.where(ok, s_sel, 0.0) - s_sel[:, :1]) * P.scale_a(tau), 0.0)
    dw = np.abs(x).max(axis=1) * U * np.log(2.0) + ULP
    rw, rv = 2.0 * dw + (k + 1) * U, 2.0 * dw + (2 * k + 1) * U
    flat = np.abs(case["segs"].astype(np.float64)).reshape(-1, C)
    A = np.einsum("qk,qkc->qc", wn, flat[np.where(ok, g_sel, 0)])
    flush = 2.0 ** -126
    return dict(g=g_sel, s=s_sel, count=count, wn=wn, V=V, bar_w=wn * (rw / (1.0 - rw))[:, None] + flush,
                bar_v=A * (rv / (1.0 - rv))[:, None] + k * flush * float(flat.max()),
                x_min=float(np.where(ok, (np.where(ok, s_sel, 0.0) - s_sel[:, :1]) / tau, 0.0).min()))


# ---- the fp32 emulation of the walk, with mutants ----------------------------------------------------------------------------------
# A mutant is a namespace with a `kind` and what the kind needs.  The kinds:
#   drop_lh / drop_hl       the (query lo, key hi) / (query hi, key lo) term is not added
#   add_ll                  (query lo, key lo) is added
#   chunk_zero / chunk_hi   the 8 halves that lane half `lh` reads at step `s` of the key lo pane hold zero / the hi pane's halves, in
#                           slice `dc` of every block (dc = None: in every slice, what a wrong fragment address does)
#   skip_slice              the last slice of key block `kb` is skipped
#   stale_rows              the first slice of every block after the first takes the previous block's key rows (a prefetch gone wrong)
#   pad_key                 a pad key of the ragged last block is not forced out
#   ge                      kmeans keeps the LATER of two equal scores in a lane's running pair (>= for >)
#   no_index                better() compares the scores alone
def mutant(kind, **kw):
    return types.SimpleNamespace(kind=kind, **kw)


NONE = mutant("none")
MUTANTS = [mutant("drop_lh"), mutant("drop_hl"), mutant("add_ll"), mutant("chunk_zero", dc=0, s=1, lh=1), mutant("chunk_zero", dc=None, s=3, lh=0),
           mutant("chunk_hi", dc=0, s=1, lh=1), mutant("chunk_hi", dc=None, s=2, lh=1), mutant("skip_slice", kb=1), mutant("stale_rows"),
           mutant("pad_key"), mutant("ge"), mutant("no_index")]


def mutant_id(m):
    return "-".join([m.kind] + [f"{k}{v}" for k, v in sorted(vars(m).items()) if k != "kind"])


def walk(q, k, mut=NONE, three=False):
    """The walk in fp32: q = (hi, lo) fp32 [nq, D] query rows, k = (hi, lo) fp32 [64 nkb, D] key rows as the blocks stage them (pad rows
    already the re-read real ones).  Key blocks of 64 in ascending order, per block slices of 64 halves in ascending order, per slice
    four steps of 16 halves (two 8-half chunks, one per lane half), per step the three products lo . hi, hi . lo, hi . hi, into one
    accumulator or (three: ncut) into three that are combined as (lh + hl) + hh per block.  -> fp32 [nq, 64 nkb], before the unscale.
    One numpy product of 16 halves stands for one MFMA: the order INSIDE it is numpy's, which matters to no exact probe."""
    qh, ql = q
    kh, kl = k
    nq, D = qh.shape
    nkb, ndc = kh.shape[0] // TILE, D // TILE
    out = np.zeros((nq, nkb * TILE), dtype=np.float32)
    for kb in range(nkb):
        acc = [np.zeros((nq, TILE), dtype=np.float32) for _ in range(3)]
        for dc in range(ndc):
            if mut.kind == "skip_slice" and kb == min(mut.kb, nkb - 1) and dc == ndc - 1:
                continue
            src = kb - 1 if (mut.kind == "stale_rows" and kb > 0 and dc == 0) else kb
            rows = slice(src * TILE, src * TILE + TILE)
            for s in range(4):
                cols = slice(dc * TILE + 16 * s, dc * TILE + 16 * s + 16)
                khs, kls = kh[rows, cols], kl[rows, cols].copy()
                if mut.kind in ("chunk_zero", "chunk_hi") and s == mut.s and mut.dc in (None, dc):
                    kls[:, 8 * mut.lh:8 * mut.lh + 8] = 0.0 if mut.kind == "chunk_zero" else khs[:, 8 * mut.lh:8 * mut.lh + 8]
                t = 0
                if mut.kind != "drop_lh":
                    acc[t] = acc[t] + ql[:, cols] @ khs.T
                t = 1 if three else 0
                if mut.kind != "drop_hl":
                    acc[t] = acc[t] + qh[:, cols] @ kls.T
                if mut.kind == "add_ll":
                    acc[t] = acc[t] + ql[:, cols] @ kls.T
                t = 2 if three else 0
                acc[t] = acc[t] + qh[:, cols] @ khs.T
        out[:, kb * TILE:kb * TILE + TILE] = (acc[0] + acc[1]) + acc[2]
    return out


def f32_planes(planes):
    """fp16 [2, rows, D] -> (hi, lo) fp32"""
    return planes[0].astype(np.float32), planes[1].astype(np.float32)


def pad_rows(k, index):
    return k[0][index], k[1][index]


def unscaled(acc):
    return acc * np.float32(2.0 ** -20) + np.float32(0.0)


def list_of(w):
    """which of a query's four lists a key at position w of the walk falls into: wave half kh = (w % 64) / 32, lane half lh = bit 2 of
    the row inside the half (acc_row); the merges read the lists in the order (kh, lh) = (0, 0), (0, 1), (1, 0), (1, 1)"""
    c = w % TILE
    return (c // 32) * 2 + ((c % 32) >> 2 & 1)


def emu_kmeans(points, cplanes, mut=NONE, guard=64):
    """points fp16 [B, 2, n, D], cplanes fp16 [2, K, D] -> (scores fp32 flat [N K + guard] preset to NaN, assign int64 [N], best fp32 [N]).
    A lane's running pair takes its centroids in ascending order under a strict >; the four pairs of a point meet under better()."""
    B, _, n, D = points.shape
    K, N = cplanes.shape[1], B * n
    q = (points[:, 0].reshape(N, D).astype(np.float32), points[:, 1].reshape(N, D).astype(np.float32))
    nkb = -(-K // TILE)
    index = np.minimum(np.arange(nkb * TILE), K - 1)
    s = unscaled(walk(q, pad_rows(f32_planes(cplanes), index), mut))
    live = nkb * TILE if mut.kind == "pad_key" else K
    flat = np.full((N * K + guard,), np.nan, dtype=np.float32)
    if live > K:                                                        # (a pad centroid's score lands K .. further on in the array)
        at = (np.arange(N)[:, None] * K + np.arange(K, live)[None, :]).ravel()
        keep = at < flat.shape[0]
        flat[at[keep]] = s[:, K:live].ravel()[keep]
    flat[:N * K] = s[:, :K].ravel()
    j = np.arange(live)
    bs, bj = np.full((4, N), -np.inf, dtype=np.float32), np.full((4, N), INT_MAX, dtype=np.int64)
    for L in range(4):
        mine = j[list_of(j) == L]
        if mine.size == 0:
            continue
        sl = s[:, mine]
        pick = sl.shape[1] - 1 - np.argmax(sl[:, ::-1], axis=1) if mut.kind == "ge" else np.argmax(sl, axis=1)
        bs[L], bj[L] = sl[np.arange(N), pick], mine[pick]
    s_best, j_best = bs[0].copy(), bj[0].copy()
    for L in range(1, 4):
        take = bs[L] > s_best
        if mut.kind != "no_index":
            take |= (bs[L] == s_best) & (bj[L] < j_best)
        s_best, j_best = np.where(take, bs[L], s_best), np.where(take, bj[L], j_best)
    return flat, j_best, s_best


def emu_graph(planes, taus, mut=NONE):
    """planes fp16 [2, n, D] of one frame, a list of thresholds -> bool [T, n, 64 W]: bit (i, w) = key w is a real one and s > tau
    (the walk is emulated once: the thresholds differ in the comparison alone)"""
    n = planes.shape[1]
    nkb = -(-n // TILE)
    p = f32_planes(planes)
    s = unscaled(walk(p, pad_rows(p, np.minimum(np.arange(nkb * TILE), n - 1)), mut, three=True))
    kvalid = np.ones(nkb * TILE, dtype=bool) if mut.kind == "pad_key" else np.arange(nkb * TILE) < n
    return np.stack([kvalid[None, :] & (s > np.float32(tau)) for tau in taus])


def _top(cands, k, mut):
    """the k best of a lane's list [(s, g)] in arrival order: the total order, or (no_index) the scores alone with ties in arrival order"""
    key = (lambda c: -c[0]) if mut.kind == "no_index" else (lambda c: (-c[0], c[1]))
    return sorted(cands, key=key)[:k]


def _merge4(lists, k, mut):
    heads, out = [0, 0, 0, 0], []
    for _ in range(k):
        best = None
        for L in range(4):
            c = lists[L][heads[L]] if heads[L] < len(lists[L]) else (-np.inf, INT_MAX)
            if best is None:
                best, which = c, L
            elif c[0] > best[0] or (mut.kind != "no_index" and c[0] == best[0] and c[1] < best[1]):
                best, which = c, L
        heads[which] += 1
        out.append(best)
    return out


def emu_propagate(tq, ctx, hp, wp, R, k, mut=NONE):
    """tq fp16 [2, n, D], ctx fp16 [n_ctx, 2, n, D] -> topk int64 [n, k] in rank order, -1 beyond the candidates.  Per (8 x 8 query
    tile, context frame): the tile's window of keys in blocks of 64, a lane's list per (query, wave half, lane half), the 4-way merge
    under better(); then the k best of a query's n_ctx k candidates under the merge launch's own 64-bit keys (always the total order)."""
    n, n_ctx = hp * wp, ctx.shape[0]
    tqf = f32_planes(tq)
    cands = [[] for _ in range(n)]
    for ci in range(n_ctx):
        cf = f32_planes(ctx[ci])
        for r0 in range(0, hp, 8):
            for c0 in range(0, wp, 8):
                wr0, wr1 = max(r0 - R, 0), min(min(r0 + 7, hp - 1) + R, hp - 1)
                wc0, wc1 = max(c0 - R, 0), min(min(c0 + 7, wp - 1) + R, wp - 1)
                ww = wc1 - wc0 + 1
                nkeys = ww * (wr1 - wr0 + 1)
                nkb = -(-nkeys // TILE)
                w = np.arange(nkb * TILE)
                wk = np.where(w < nkeys, w, 0)
                rows = (wr0 + wk // ww) * wp + wc0 + wk % ww
                qi = np.arange(64)
                qr, qc = np.minimum(r0 + qi // 8, hp - 1), np.minimum(c0 + qi % 8, wp - 1)
                qrows = qr * wp + qc
                s = unscaled(walk((tqf[0][qrows], tqf[1][qrows]), (cf[0][rows], cf[1][rows]), mut))
                kr, kc = wr0 + w // ww, wc0 + w % ww                    # (as the kernel forms them, pad keys included)
                live = nkb * TILE if mut.kind == "pad_key" else nkeys
                for t in range(64):
                    r, c = r0 + t // 8, c0 + t % 8
                    if r >= hp or c >= wp:
                        continue
                    near = (np.abs(kr[:live] - r) <= R) & (np.abs(kc[:live] - c) <= R)
                    lists = [[], [], [], []]
                    for x in np.flatnonzero(near):
                        lists[list_of(x)].append((float(s[t, x]), int(ci * n + kr[x] * wp + kc[x])))
                    cands[r * wp + c] += _merge4([_top(l, k, mut) for l in lists], k, mut)
    out = np.full((n, k), -1, dtype=np.int64)
    for q in range(n):
        real = sorted((c for c in cands[q] if c[1] != INT_MAX), key=lambda c: (-c[0], c[1]))[:k]
        out[q, :len(real)] = [c[1] for c in real]
    return out


# ---- the bars of the fp64 tests, restated (what they let through) -----------------------------------------------------------------
def unit_planes(seed, rows, D):
    """fp16 [2, rows, D]: the planes of random unit rows as normalize_tokens leaves them (tests/kmeans_util.py: split_planes)"""
    x = KM.unit_rows(np.random.default_rng(seed).standard_normal((rows, D)))
    return KM.split_planes(x.astype(np.float32))


def old_bars_pass(s, planes, k=5, tau=0.0):
    """The E / 2E checks of tests/test_kmeans_gpu.py, tests/test_ncut_gpu.py and tests/test_propagate_gpu.py applied to an emulated
    score matrix s fp32 [n, n] of one set of unit rows against itself -> dict(scores: every |s - fp64| <= E; assign: every row whose
    two best fp64 scores are more than 2E apart takes the host's column, every other one a column within 2E of the best; graph: every
    pair with |fp64 - tau| > 2E has the host's bit; topk: every row whose fp64 gap at the cut exceeds 2E selects the host's set;
    undecided: the largest share of rows or pairs that the reference leaves undecided (a property of the inputs, the same for
    every mutant; the fp64 tests cap it at 4 % on theirs); err: max |s - fp64|)"""
    D = planes.shape[2]
    E = KM.score_bar(D)
    X = KM.plane_values(planes)
    ref = X @ X.T + 0.0
    n = ref.shape[0]
    s64 = s[:, :n].astype(np.float64)
    err = float(np.abs(s64 - ref).max())
    srt = np.sort(ref, axis=1)
    dec_a = srt[:, -1] - srt[:, -2] > 2.0 * E
    a = np.argmax(s64, axis=1)
    assign = np.array_equal(a[dec_a], np.argmax(ref, axis=1)[dec_a]) and bool(np.all(ref[np.arange(n), a] >= srt[:, -1] - 2.0 * E))
    dec_g = np.abs(ref - tau) > 2.0 * E
    graph = np.array_equal((s64 > tau)[dec_g], (ref > tau)[dec_g])
    dec_k = srt[:, -k] - srt[:, -k - 1] > 2.0 * E
    top_d, top_h = np.sort(np.argsort(-s64, axis=1, kind="stable")[:, :k], axis=1), np.sort(np.argsort(-ref, axis=1, kind="stable")[:, :k], axis=1)
    topk = np.array_equal(top_d[dec_k], top_h[dec_k])
    undecided = float(max(1.0 - dec_a.mean(), 1.0 - dec_g.mean(), 1.0 - dec_k.mean()))
    return dict(scores=err <= E, assign=assign, graph=graph, topk=topk, undecided=undecided, err=err, E=E)


# ---- the probe checks, shared by the emulation (tests/test_pair_probes_cpu.py) and the device (tests/test_pair_probes_gpu.py) --------
def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float32).view(np.uint32), np.ascontiguousarray(b, dtype=np.float32).view(np.uint32))


def kmeans_failures(ref, scores_flat, assign, best):
    """scores_flat: fp32 [N K + guard], the guard still holding the NaN it was preset to -> the list of what is wrong (empty: nothing)"""
    N, K = ref["S"].shape
    bad = []
    if not same_bits(scores_flat[:N * K].reshape(N, K), ref["scores"]):
        bad.append("scores differ from the exact ones")
    if not np.all(np.isnan(scores_flat[N * K:])):
        bad.append("something was written past the scores")
    if not np.array_equal(np.asarray(assign, dtype=np.int64), ref["assign"]):
        bad.append("assign is not the first maximum")
    if not same_bits(best, ref["best"]):
        bad.append("best is not the selected score")
    return bad


def graph_failures(S, thresholds, bits):
    """S int64 [n, n], bits bool [T, n, 64 W] at the integer thresholds t (tau = (t + 1/2) 2^(2e - 20)): bit = S > t + 1/2"""
    n = S.shape[0]
    bad = []
    if bits[:, :, n:].any():
        bad.append("a pad bit is set")
    real = bits[:, :, :n]
    if not np.array_equal(real, real.transpose(0, 2, 1)):
        bad.append("the graph is not symmetric")
    want = S[None, :, :] > np.asarray(thresholds, dtype=np.int64)[:, None, None]
    if not np.array_equal(real, want):
        counts = real.sum(axis=0)
        bad.append(f"{int((counts != want.sum(axis=0)).sum())} pairs read back another score; {int((real != want).sum())} bits differ")
    return bad


def indicator_failures(u, w, bits):
    """bits bool [n, 64 W] at IND_TAU"""
    n = u.shape[0]
    hh, hl, lh, _ = indicator_terms(u, w)
    bad = []
    if bits[:, n:].any():
        bad.append("a pad bit is set")
    if not np.array_equal(bits[:, :n], hh | hl | lh):
        bad.append(f"{int((bits[:, :n] != (hh | hl | lh)).sum())} indicator bits differ")
    return bad


def topk_failures(ref, idx):
    k = ref["g"].shape[1]
    bad = []
    idx = np.asarray(idx, dtype=np.int64)
    if not np.array_equal(idx, ref["g"]):
        bad.append(f"topk_idx differs from the ranked reference at {int((idx != ref['g']).any(axis=1).sum())} queries")
    if not np.array_equal(idx >= 0, np.arange(k)[None, :] < np.minimum(ref["count"], k)[:, None]):
        bad.append("-1 does not sit exactly beyond the candidates")
    return bad
