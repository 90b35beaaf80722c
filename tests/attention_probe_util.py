"""Exact probes and per-element bounds for the attention forward kernels (tests/test_attention_probes_gpu.py, ..._cpu.py).

dinoseg_op_attention takes q already scaled into the log2 domain: the kernel's score is q.k itself and a probability is 2^score.  On random
draws the kernels (attention.hip, attention_z.hip, attention_za.hip) can only be held to one maximum-error bar per tensor, and any key
whose probability x |v| is below that bar can be dropped, counted twice or mis-weighted unseen.  Here the inputs are chosen so that every
intermediate is exact in every route's arithmetic -- small integers, integer scores, probabilities that are powers of two or exactly zero,
row sums and P.V sums within 24 bits -- so that the result does not depend on tile order, wave-group split or rescale history, and the
expected output is an exact rational computed with integers.  Host side only: numpy, and torch on the CPU for nothing but the bf16 / fp16
conversions (as tests/probe_util.py); nothing touches the GPU and nothing is read from outside the repository.

Construction.  Key j carries the +-1 code of the 12 bits of its code value (j + rot) mod ntok on 12 of the 64 head dimensions; two more
dimensions carry offsets; which 14 they are is a rotation of one seeded permutation by 14 per case (case_dims), so that five consecutive
cases use every dimension.  Per query and bit:
  hard       q = +-A (A = 128) with the sign of the wanted bit; the offset dimension holds q = 1, k = -A * (number of hard bits): the score is
             -2 A * (mismatched hard bits), 0 on a match and <= -256 otherwise.  2^-256 is exactly 0 in fp32, bf16 and fp16, and so is a
             rescale by 2^-256 in the kernels that keep a running reference (their reference trails the row maximum by at most 16, and
             2^(-256 + 16 + 8) is still below fp32's smallest subnormal 2^-149; with the shifts of the zero-reference kernels' fast path,
             |c| <= 60, the absolute score stays below -190).
  don't care q = 0: the selected set is every existing key that matches on the cared bits.
  soft       q = +-1/2: the score loses exactly 1 per mismatch, P = 2^-h relative to the best key.  The weights probe makes the six high
             index bits soft wherever the index has six bits (33 tokens on; 2 ^ 6 = 64 weighted neighbours where that many keys exist); the
             number of soft bits is even, so that the scores stay integers.
  shift      the second offset dimension holds q = 1 and k = c: the integer c is added to every row's scores.  For a shift of ONE row a
             fifteenth dimension holds q = 1 in that row alone and k = c in every key.
V holds small nonzero integers that depend on (batch, head, key, d).  On hi + lo routes V needs two planes (512 u + w on bf16 planes,
4096 u + w on fp16 planes, w odd: no value fits one plane) and either K or Q has a lo plane that changes which keys weigh what:
  "k"  the shift dimension of K holds 4096 + c - e_j and the offset dimension -4096 more; e_j in {0, 1} is a per-key bit that only the lo
       plane carries;
  "q"  the shift dimension of Q holds 1 + 2^-12, K holds 4096 (1 + e_j) there and -4096 (1 + e_j) more on the offset dimension;
never both factors of one product (the kernels drop lo x lo by design).  Pad rows ntok..npad of K repeat a real key that some query
selects, pad rows of V hold large integers, pad rows of Q repeat query 0: a masked pad key must change no bit (include/dinoseg.h).

Bounds (derived from the epilogues; nothing is fitted to an output).
  Every kernel ends in  inv = 1.0f / l_tot;  x = o * inv;  store(x)  with o and l_tot exact here.
  * l_tot a power of two: inv and x are exact in fp32 (x has at most 24 significant bits: asserted per case), so the stored planes are
    the round-to-nearest-even planes of the exact rational: BIT EQUALITY (split_bf16x2 / split2 / pack2 of common.h round to nearest even:
    hi = RNE(x), lo = RNE(x - hi) with x - hi exact).
  * otherwise  |got - exact| <= h(exact) + 4 * 2^-24 |exact|.  h is the store format's own rounding (half_ulp_store): one plane half an ulp,
    2^(e - 8) for bf16 and 2^(max(e, -14) - 11) for fp16 at |x| in [2^e, 2^(e+1)); hi + lo planes 2^(e - 17) for bf16 (|x - hi| <= 2^(e - 8)
    is below 2^(e - 8), so the lo plane's half ulp is at most 2^(e - 9 - 8)) and max(2^(e - 23), 2^-25) for fp16 (the same with 11 bits;
    2^-25 is half an fp16 subnormal step, common.h split2).  These are the per-binade figures; they are never above the relative ones
    (2^-8, 2^-11, 2^-16, 2^-22) and the CPU test shows by brute force that they are reached to 0.9.  The fp32 term: the division is
    compiled without fast-math flags, so 1.0f / l_tot is correctly rounded (2^-24); were it a bare v_rcp_f32 (one ulp, 2^-23 relative
    at worst) plus the multiply (2^-24) the sum is 3 * 2^-24: 4 * 2^-24 covers both, and the move of the store rounding's binade.
  * lse = m_ref + v_log_f32(l_tot).  Neither the ISA description nor common.h states an accuracy for v_log_f32: it is ASSUMED, not
    measured, to be 2 ulps of fp32 at the magnitude of its result r.  r is lse itself in the zero-reference kernels' fast path,
    log2(l) in [0, 12] on their exact path, and lse - m_run with m_run trailing the row maximum by at most `trail` (16; 14 on fp16
    planes: RESCALE_THR of attention.hip) in the kernels with a running reference, so |r| <= R = max(|lse|, log2(l_rel) + trail).  The
    add of the integer m_ref rounds once, half an ulp at |lse|, and half an ulp more is the result's own representation:
        |got - exact| <= 2 ulp(R) + ulp(|lse|),  ulp(x) = 2^(floor(log2 x) - 23)   (lse_bound; 2^-149 where x = 0).
    Slack that is left in: R is the larger of the results the routes' paths can log, not the one result of the path a row took.  Which
    path a zero-reference row takes is decided by the other rows of its workgroup, so a fast-path row (r = lse) is also allowed the 2 ulps
    at log2(l); that is wider than 2 ulps at |lse| only where |lse| < log2(l), i.e. for negative shifts no larger than log2(l) <= 12.  On
    the running-reference routes a row with lse = 0 is allowed 2 ulp(trail) = 2^-18, because its log's result is lse - m_run, up to trail.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field
from fractions import Fraction

import numpy as np
import torch

A = 128.0                    # the hard bits' query magnitude
NBITS = 12                   # code bits: ntok <= 4096
G = 4096.0                   # what makes the shift dimension need two planes on hi + lo routes
HMAX = 8                     # probabilities are kept as integers 2^(HMAX - h), h = distance below the row's best score
ZERO_FROM = 240              # every other key lies at least this far below the best one: exactly 0 in every route
SHIFTS = (0, 1, -1, 59, -59, 60, -60, 61, -61, 126, -126, 200, -200)
PROBES = ("selector", "groups", "weights", "count")
_BASE_PERM = np.random.default_rng(20240).permutation(64)


def case_dims(n: int) -> np.ndarray:
    """the 14 head dimensions case n uses: 12 code dimensions, the hard-bit offset, the shift"""
    return np.roll(_BASE_PERM, -14 * n)[:14]


def coprime_steps(ntok: int):
    """(s, t) of the permutations i -> (s i + t) mod ntok: the identity (partner in the query's own tile), a reversal (early <-> late) and
    a stride near ntok / 2 (far tiles), each made coprime to ntok"""
    out = [(1, 0)]
    for s0, t in ((ntok - 1, 5), (ntok // 2 + 1, ntok // 3)):
        s = max(1, s0)
        while math.gcd(s, ntok) != 1:
            s += 1
        st = (s % ntok if ntok > 1 else 1, t % ntok)
        if st not in out:
            out.append(st)
    return out


@dataclass
class Case:
    probe: str
    B: int
    H: int
    ntok: int
    npad: int
    Q: np.ndarray                 # [B, H, npad, 64] fp64, exact values
    K: np.ndarray
    V: np.ndarray
    ctx: np.ndarray               # [B * ntok, H * 64] fp64: num / den, exact where pow2
    num: np.ndarray               # [B * ntok, H * 64] int64: sum of 2^(HMAX - h) v
    den: np.ndarray               # [B * ntok, H] int64: sum of 2^(HMAX - h)
    pow2: np.ndarray              # [B * ntok, H] bool: den is a power of two -> bit equality
    lse: np.ndarray               # [B, H, ntok] fp64
    log2l: np.ndarray             # [B, H, ntok] fp64: log2 of the row sum relative to the row's best score
    dims: np.ndarray
    sh_col: int
    qsh: np.ndarray               # [ntok] what the shift dimension of Q holds (the same in every pair)
    meta: dict = field(default_factory=dict)


def _v_values(g, shape, planes, v_fp16):
    w = g.integers(1, 128, shape) * np.where(g.integers(0, 2, shape) == 0, 1, -1)
    if planes == 1:
        return w.astype(np.float64)
    w = w | 1                                                   # odd: the lo plane is never empty
    sign = np.where(g.integers(0, 2, shape) == 0, 1, -1)
    u = sign if v_fp16 else sign * g.integers(1, 3, shape)
    return ((4096 if v_fp16 else 512) * u + w).astype(np.float64)


def soft_bits(ntok: int):
    nb = max(ntok - 1, 0).bit_length()
    ns = min(6, nb) // 2 * 2             # six wherever the index has six bits; even, so that a full match scores the integer ns / 2
    return list(range(nb - ns, nb))


def build(probe, B, H, ntok, n=0, s=1, t=0, rot=0, planes=1, v_fp16=False, lo=None, seed=0, expect=True) -> Case:
    """One probe at shift c = 0 (shifted() derives the others).  lo: None, "k" or "q" (hi + lo routes, selector and weights only).
    expect = False: the operands alone (tests/attention_bwd_probe_util.py takes Q and K from here and has expectations of its own)."""
    assert probe in PROBES and 1 <= ntok <= 1 << NBITS and math.gcd(s, ntok) == 1
    assert lo is None or (planes == 2 and probe in ("selector", "weights"))
    npad = (ntok + 63) // 64 * 64
    dims = case_dims(n)
    code_d, off_d, sh_d = dims[:NBITS], int(dims[NBITS]), int(dims[NBITS + 1])
    g = np.random.default_rng([seed, B, H, ntok, n, planes, int(v_fp16)])
    j = np.arange(ntok)
    code = (j + rot) % ntok
    bits = (((code[:, None] >> np.arange(NBITS)) & 1) * 2 - 1).astype(np.float64)          # [ntok, 12]
    i = np.arange(ntok)
    kind = np.full((ntok, NBITS), 2)                                                       # 2 hard, 1 soft, 0 don't care
    if probe == "groups":
        b1 = i % NBITS
        b2 = (b1 + 1 + (i // NBITS) % (NBITS - 1)) % NBITS
        kind[i, b1] = 0
        kind[i, b2] = 0
    elif probe == "weights":
        kind[:, soft_bits(ntok)] = 1
    elif probe == "count":
        kind[:] = 0
    nh = int((kind[0] == 2).sum())
    assert ((kind == 2).sum(axis=1) == nh).all()
    qmag = np.where(kind == 2, A, np.where(kind == 1, 0.5, 0.0))
    e = ((j * 2654435761 >> 7) & 1).astype(np.float64) if lo else np.zeros(ntok)
    Q, K = np.zeros((B, H, npad, 64)), np.zeros((B, H, npad, 64))
    V = np.zeros((B, H, npad, 64))
    V[:, :, :ntok] = _v_values(g, (B, H, ntok, 64), planes, v_fp16)
    V[:, :, ntok:] = (96 + np.arange(64) % 7) * 256.0
    pis = np.zeros((B, H, ntok), dtype=np.int64)
    for b in range(B):
        for h in range(H):
            pi = (s * i + t + 7 * (b * H + h)) % ntok
            pis[b, h] = pi
            q, k = Q[b, h], K[b, h]
            k[:ntok, code_d] = bits
            if probe != "count":
                q[:ntok, code_d] = bits[pi] * qmag
                q[:ntok, off_d] = 1.0
                q[:ntok, sh_d] = 1.0 + 2.0 ** -12 if lo == "q" else 1.0
            k[:ntok, off_d] = -A * nh - (G * (1.0 + e) if lo == "q" else G if lo == "k" else 0.0)
            k[:ntok, sh_d] = G * (1.0 + e) if lo == "q" else G - e if lo == "k" else 0.0
            k[ntok:] = k[pi[ntok // 2]]
            q[ntok:] = q[0]
    c = Case(probe, B, H, ntok, npad, Q, K, V, None, None, None, None, None, None, dims, sh_d, Q[0, 0, :ntok, sh_d].copy(),
             {"pi": pis, "kind": kind, "nh": nh, "n": n, "code": code, "lo": lo, "planes": planes, "v_fp16": v_fp16})
    if expect:
        _expect(c)
    return c


def _expect(c: Case):
    """the exact expectations, from the VALUES of Q, K and V (not from the construction: the CPU test holds the construction's claims
    against them): integer scores, integer probabilities 2^(HMAX - h), integer sums"""
    B, H, ntok = c.B, c.H, c.ntok
    num = np.zeros((B, ntok, H, 64), dtype=np.int64)
    den = np.zeros((B, ntok, H), dtype=np.int64)
    lse, log2l = np.zeros((B, H, ntok)), np.zeros((B, H, ntok))
    nsel = np.zeros((B, H, ntok), dtype=np.int64)
    hit = np.zeros((B, H, ntok), dtype=np.int64)
    for b in range(B):
        for h in range(H):
            S = c.Q[b, h, :ntok] @ c.K[b, h, :ntok].T                   # exact in fp64: dyadic operands of a few bits
            m = S.max(axis=1)
            hrel = m[:, None] - S
            assert (hrel == np.round(hrel)).all() and (m == np.round(m)).all(), "scores are integers"
            near = hrel <= HMAX
            assert (near | (hrel >= ZERO_FROM)).all(), "a key is neither weighted nor exactly zero"
            P = np.where(near, 2.0 ** (HMAX - np.minimum(hrel, HMAX)), 0.0)
            d = P.sum(axis=1)
            Vr = c.V[b, h, :ntok]
            o = P @ Vr
            unit = np.where(near, P, np.inf).min(axis=1)                # the row's smallest nonzero probability: every term is a multiple
            assert ((P @ np.abs(Vr)).max(axis=1) / unit < 2.0 ** 24).all() and (d / unit < 2.0 ** 24).all(), "a partial sum leaves 24 bits"
            num[b, :, h], den[b, :, h] = o.astype(np.int64), d.astype(np.int64)
            assert (num[b, :, h] == o).all() and (den[b, :, h] == d).all()
            log2l[b, h] = np.log2(d) - HMAX
            lse[b, h] = m + log2l[b, h]
            nsel[b, h] = near.sum(axis=1)
            hit[b, h] = near.sum(axis=0)
    c.num, c.den = num.reshape(B * ntok, H * 64), den.reshape(B * ntok, H)
    c.pow2 = (c.den & (c.den - 1)) == 0
    c.ctx = c.num.astype(np.float64) / np.repeat(c.den, 64, axis=1)
    ex = np.repeat(c.pow2, 64, axis=1)
    assert (c.ctx[ex] * np.repeat(c.den, 64, axis=1)[ex] == c.num[ex]).all(), "a power-of-two quotient converts exactly"
    c.lse, c.log2l = lse, log2l
    c.meta.update(nsel=nsel, hit=hit)


def shifted(c: Case, shift: int, one_row=None):
    """(Q, K, lse) of the same case with the integer `shift` added to every score of every row (K's shift dimension holds `shift` more:
    not with a lo plane in Q, whose 1 + 2^-12 there would make it a fraction), or of row `one_row` alone: a fifteenth dimension, unused by
    the case, holds q = 1 in that row only and k = shift in every key, whatever the lo planes of the other dimensions do (it has none of
    its own).  ctx is unchanged by construction."""
    Q, K = c.Q, c.K.copy()
    add = np.ones(c.ntok)
    if one_row is not None:
        row_d = int(np.roll(_BASE_PERM, -14 * c.meta["n"])[NBITS + 2])
        assert row_d not in c.dims and not c.Q[..., row_d].any() and not c.K[..., row_d].any()
        Q = c.Q.copy()
        Q[:, :, one_row, row_d] = 1.0
        K[:, :, :, row_d] = shift
        add = np.zeros(c.ntok)
        add[one_row] = 1.0
    else:
        assert c.meta["lo"] != "q" or shift == 0
        K[:, :, :, c.sh_col] += shift
    return Q, K, c.lse + shift * add[None, None, :]


def case_list(shapes, planes=1):
    """The probes of one route: [(probe, (B, H, ntok), build keywords, shifted too)] with a running case number n (-> case_dims: every
    five consecutive cases use all 64 dimensions).  Selector: every (s, t) of coprime_steps; groups: the first two; weights: the far stride
    at two code rotations (the best key of a query arrives in the first, a middle or the last tile, depending on the query); count.  On
    hi + lo routes the variants alternate between a lo plane in K and in Q.  Long sequences (more than 1024 tokens) take one variant of
    each.  One selector and one weights variant without a lo plane in Q also run at every shift."""
    out, n = [], 0
    for shp in shapes:
        ntok = shp[2]
        steps = coprime_steps(ntok)
        lean = ntok > 1024
        los = [None] if planes == 1 else ["k", "q"]
        far = steps[-1]
        variants = {
            "selector": [dict(s=s, t=t, lo=los[i % len(los)]) for i, (s, t) in enumerate(steps[-1:] if lean else steps)],
            "groups": [dict(s=s, t=t) for s, t in (steps[-1:] if lean else steps[:2])],
            "weights": [dict(s=far[0], t=far[1], rot=r, lo=los[i % len(los)]) for i, r in enumerate((0,) if lean else (0, ntok // 3))],
            "count": [dict()],
        }
        for probe in PROBES:
            for i, kw in enumerate(variants[probe]):
                out.append((probe, shp, dict(kw, n=n, planes=planes), i == 0 and probe in ("selector", "weights")))
                n += 1
    return out


# ------------------------------------------------------------------------------------------------ number formats and bounds
def tdtype(fp16: bool):
    return torch.float16 if fp16 else torch.bfloat16


def rne_planes(x: np.ndarray, fp16: bool, planes: int) -> np.ndarray:
    """fp64 values that fp32 holds exactly -> int16 planes [planes, ...]: hi = RNE(x), lo = RNE(x - hi) (what common.h's splits write)"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float32))
    assert (t.double().numpy() == x).all(), "not an fp32 value"
    dt = tdtype(fp16)
    hi = t.to(dt)
    pl = [hi] if planes == 1 else [hi, (t - hi.float()).to(dt)]
    return torch.stack(pl).contiguous().view(torch.int16).numpy()


def planes_value(p: np.ndarray, fp16: bool) -> np.ndarray:
    return torch.from_numpy(np.ascontiguousarray(p)).view(tdtype(fp16)).double().sum(dim=0).numpy()


def exact_planes(x: np.ndarray, fp16: bool, planes: int) -> np.ndarray:
    """operand planes of exact values: asserts that the format holds them without loss"""
    p = rne_planes(x, fp16, planes)
    assert (planes_value(p, fp16) == x).all(), f"an operand is not exact in {planes} {'fp16' if fp16 else 'bf16'} plane(s)"
    return p


def half_ulp_store(mag, fp16: bool, planes: int) -> np.ndarray:
    """what the store may lose at magnitude mag in [2^e, 2^(e+1)) (the docstring above)"""
    mag = np.maximum(np.abs(np.asarray(mag, dtype=np.float64)), 2.0 ** -140)
    e = np.floor(np.log2(mag))
    if planes == 1:
        return 2.0 ** (np.maximum(e, -14.0) - 11.0) if fp16 else 2.0 ** (e - 8.0)
    return np.maximum(2.0 ** (e - 23.0), 2.0 ** -25) if fp16 else 2.0 ** (e - 17.0)


def ctx_bound(exact, fp16: bool, planes: int) -> np.ndarray:
    return half_ulp_store(exact, fp16, planes) + 4.0 * 2.0 ** -24 * np.abs(exact)


def ulp32(x) -> np.ndarray:
    x = np.abs(np.asarray(x, dtype=np.float64))
    return 2.0 ** (np.floor(np.log2(np.maximum(x, 2.0 ** -126))) - 23.0)


def lse_bound(lse, log2l, trail: int) -> np.ndarray:
    """2 ulp(R) + ulp(|lse|), R = max(|lse|, log2(l) + trail) -- the v_log_f32 figure is assumed (the docstring above)"""
    R = np.maximum(np.abs(lse), np.abs(log2l) + trail)
    return np.where(R == 0.0, 0.0, 2.0 * ulp32(R)) + np.where(np.asarray(lse) == 0.0, 2.0 ** -149, ulp32(lse))


def fraction_ctx(c: Case, row: int, col: int) -> Fraction:
    return Fraction(int(c.num[row, col]), int(c.den[row, col // 64]))


# ------------------------------------------------------------------------------------------------ fp32 emulation of the two bookkeepings
F32 = np.float32
KB = 64


def _exp2(s):
    """2^s in fp32 for integer-valued s: exact, inf above 127, subnormal / 0 below -126 (v_exp_f32 on an integer)"""
    with np.errstate(over="ignore", under="ignore"):
        return np.ldexp(F32(1.0), np.clip(s, -400, 400).astype(np.int64)).astype(F32)


def _tiles(ntok, order, groups):
    nt = (ntok + KB - 1) // KB
    ts = list(range(nt))
    if order == "reversed":
        ts = ts[::-1]
    chunk = (nt + groups - 1) // groups
    return [ts[g * chunk:(g + 1) * chunk] for g in range(groups)]


def emulate_zero_reference(q, k, v, ntok, order="natural", groups=1):
    """attention_z.hip in fp32 numpy, one (batch, head) pair, every query at once: probabilities 2^S against the reference 0, partial O and l
    of the wave groups added; a row sum outside [2^-60, 2^60] sends ALL rows through the two-pass recomputation (maxima, then 2^(S - max)).
    Returns (O, l, m_ref) before the final divide."""
    q, k, v = (np.asarray(x, dtype=F32) for x in (q, k, v))
    n = q.shape[0]

    def sweep(tiles, m):
        o, l = np.zeros((n, 64), F32), np.zeros(n, F32)
        with np.errstate(over="ignore", invalid="ignore"):
            for t in tiles:
                ks = slice(t * KB, min((t + 1) * KB, ntok))
                p = _exp2(q @ k[ks].T - m[:, None])
                l = l + p.sum(axis=1, dtype=F32)
                o = o + p @ v[ks]
        return o, l
    parts = [sweep(ts, np.zeros(n, F32)) for ts in _tiles(ntok, order, groups)]
    o, l = parts[0]
    with np.errstate(over="ignore", invalid="ignore"):
        for po, pl in parts[1:]:
            o, l = o + po, l + pl
    m = np.zeros(n, F32)
    if not ((l >= F32(2.0 ** -60)) & (l <= F32(2.0 ** 60))).all():
        ts = [t for grp in _tiles(ntok, order, 1) for t in grp]
        m = np.max(np.stack([(q @ k[t * KB:min((t + 1) * KB, ntok)].T).max(axis=1) for t in ts]), axis=0).astype(F32)
        o, l = sweep(ts, m)
    return o, l, m


def emulate_running_reference(q, k, v, ntok, order="natural", groups=1, thr=16.0):
    """attention.hip in fp32 numpy: scores against a running reference that the first tile sets to its row maximum and that moves (for every
    row, by max(row maximum, 0)) when any row's tile maximum exceeds it by more than thr; O and l are rescaled then.  Wave groups (a split
    this file does not have in the kernels: it shows the order independence) are merged at the larger reference.  Returns (O, l, m_run)."""
    q, k, v = (np.asarray(x, dtype=F32) for x in (q, k, v))
    n = q.shape[0]

    def sweep(tiles):
        o, l, m = np.zeros((n, 64), F32), np.zeros(n, F32), np.zeros(n, F32)
        for idx, t in enumerate(tiles):
            ks = slice(t * KB, min((t + 1) * KB, ntok))
            s = q @ k[ks].T - m[:, None]
            mx = s.max(axis=1)
            if idx == 0 or (mx > thr).any():
                delta = mx if idx == 0 else np.maximum(mx, F32(0.0))
                alpha = np.ones(n, F32) if idx == 0 else _exp2(-delta)
                m, l, o, s = m + delta, l * alpha, o * alpha[:, None], s - delta[:, None]
            p = _exp2(s)
            l = l + p.sum(axis=1, dtype=F32)
            o = o + p @ v[ks]
        return o, l, m
    parts = [sweep(ts) for ts in _tiles(ntok, order, groups) if ts]
    o, l, m = parts[0]
    for po, pl, pm in parts[1:]:
        mm = np.maximum(m, pm)
        a, b = _exp2(m - mm), _exp2(pm - mm)
        o, l, m = o * a[:, None] + po * b[:, None], l * a + pl * b, mm
    return o, l, m
