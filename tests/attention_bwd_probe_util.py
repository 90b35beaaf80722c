"""Exact probes of the attention backward (attention_bwd.hip) -- host side only: numpy, and torch on the CPU for the bf16 conversions.

dinoseg_op_attention_bwd takes lse and O as inputs, so a probe supplies all six operands (Q~, K, V, dO, O, lse) and never runs the forward.
The kernels compute, from those inputs and nothing else (the header comment of attention_bwd.hip),
    delta = sum_d dO O,   P = 2^(Q~.K^T - lse),   dP = dO.V^T,   dS = P (dP - delta),   dQ = 0.125 dS.K,   dK = ln2 dS^T.Q~,   dV = P^T.dO
and here every one of these is exact in the kernels' arithmetic, so the expected planes are a property of the inputs: whatever the tile
order, the wave <-> row mapping or the accumulation order, dQ and dV must be THE round-to-nearest-even planes of 0.125 * sum and of the sum,
bit for bit on both planes, and dK -- the epilogue's  float32(sum) * float32(ln 2)  of an exact sum -- on one plane the RNE plane of that one
IEEE product, bit for bit.  On hi + lo planes dK is held to a bound instead:  |hi + lo - x| <= half_ulp_store(x) + 2^-23 |x|,  x the exact
product of the two fp32 factors.  Why: the split writes lo = RNE(p - hi) with p = sum * ln2, and the compiler contracts that multiply and
subtract into one fma(sum, ln2, -hi), so the lo plane is rounded from the EXACT product, not from its fp32 rounding (measured on the MI355X:
the hi planes agree, the lo planes differ from the two-step reading by one lo-plane ulp in 24 of 37 440 elements of one case).  Either
reading is a correct split; which one the compiler picks is not the kernel's contract, so neither is asserted bit for bit.  The bound is the
store format's own half ulp (tests/attention_probe_util.py) plus one fp32 ulp of the product; nothing in it is fitted.  dQ's factor 0.125
is exact under either reading, and dV has none.

Construction.  Q~ and K are those of tests/attention_probe_util.py (key codes on rotating head dimensions, hard / soft / don't-care bits,
per-key lo bits on hi + lo planes; P.build is called, not copied), so every score is an integer and every key is either within HMAX of its
row's best score or at least ZERO_FROM below it.  lse is an integer at or above the row maximum, so P is a power of two or exactly 0.
V holds small nonzero integers (|v| <= 15; |v| <= 3 where dO is wide), dO one or two nonzero integers per (frame, head, query) on dimensions
that move with all three indices, O small integers (or the true ctx).  Probes:
  selector  consistent: one key pi(q) per query, lse and O are the true log-sum-exp and ctx.  dS = 0 exactly (dP - delta = dO.(V[pi] - O)),
            dQ = dK = 0, dV[pi(q)] = dO[q]: the dV routing and the (frame, head, row) layout.
  pick      the selector's geometry with lse = max + (q mod 2) and a free O: ONE nonzero P (1 or 1/2) and one nonzero dS per query, so every
            dQ, dK, dV element is a single product.  This is where a lo plane of K or Q~ meets a nonzero dS, and where (variant
            `rounded`) dS deliberately needs MORE bits than the planes hold: the expectation states the kernels' rounding of dS to the
            planes (hi = RNE(dS), lo = RNE(dS - hi)) explicitly, which is what tells a truncating split from a rounding one.
  groups    consistent on the rows whose selected set has 1, 2 or 4 keys (lse = max + log2 n, O = the mean, multiples of 1/4); a row with 3
            keys gets lse = max + 2 and a zero dO row, so that it contributes exactly nothing under either reading.
  weights   free: the six high index bits soft, 64 neighbours at P = 2^-h, lse = max + (q mod 3), O chosen integers.
  count     free: Q~ = 0, lse = q mod 3: every key counts once in every dQ row, every query once in every dV row; dK = 0.
hi + lo planes.  Some operand of each of the five products needs its lo plane: K or Q~ for the scores (selector and pick, as in the forward
util), dO = 256 u + w (w odd) for dP and dV, O = 256 u + w on dO's second dimension for delta, a dS of more than 8 significant bits for dQ
and dK (groups, weights, count, rounded pick), and K's or Q~'s own lo plane for dQ / dK in the pick variants with a narrow dS.  NEVER both
factors of one product: the kernels multiply hi.hi + hi.lo + lo.hi and drop lo.lo, the builder asserts per output column that no dropped
term is nonzero, so the expectation is the full product, while the emulation below spells the three-product rule out -- the two agree bit
for bit only because of that assertion.  (The selector has wide dO AND a lo plane in K / Q~: its dS is exactly 0.)
Asserted per case on the VALUES: integer scores, P a power of two or 0, dS within the planes (8 / 16 significant bits; not `rounded`),
and for every sum of products sum|terms| / granule < 2^24 with the granule that of (row of the left factor) x (column of the right one), so
that every partial sum in any order is an fp32 value.
Pad rows ntok..npad: K repeats a real key that some query weights, V holds large integers, Q~ repeats query 0 (P.build)."""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np
import torch

from tests import attention_probe_util as P

F32 = np.float32
LN2 = F32(0.69314718055994530942)
PROBES = ("selector", "pick", "groups", "weights", "count")
SHAPES = [(1, 1, 1), (1, 1, 33), (1, 3, 65), (2, 2, 197), (1, 1, 257), (2, 5, 300)]
PRODUCTION = (1, 6, 3601)
MUTANTS = ("mask+1", "mask-1", "padq", "noclamp", "dq_skip", "dq_twice", "dkv_skip", "dkv_twice", "trunc", "no_ds_lo", "swap_heads",
           "no_delta", "scales")


@dataclass
class BwdCase:
    probe: str
    B: int
    H: int
    ntok: int
    npad: int
    planes: int
    Q: np.ndarray                 # [B, H, npad, 64] fp64, exact values
    K: np.ndarray
    V: np.ndarray
    dO: np.ndarray                # [B * ntok, H * 64]
    O: np.ndarray
    lse: np.ndarray               # [B, H, ntok], integers
    sums: dict = field(default_factory=dict)      # "dq" / "dk" / "dv": [B, ntok, H, 64] fp64, the exact sums before the epilogue's factor
    mags: dict = field(default_factory=dict)      # the same of |terms|
    expect: np.ndarray = None     # int16 planes [planes, B * ntok, 3 * H * 64]
    meta: dict = field(default_factory=dict)


# ------------------------------------------------------------------------------------------------ number formats
def plane_values(x, planes):
    """exact fp64 values -> (hi, lo) fp32 values of their RNE planes (lo = 0 on one plane)"""
    p = torch.from_numpy(P.rne_planes(x, False, planes)).view(torch.bfloat16).float().numpy()
    return p[0], (p[1] if planes == 2 else np.zeros_like(p[0]))


def round_to_planes(x, planes):
    """what the kernels' split keeps of fp32 values: hi = RNE(x), lo = RNE(x - hi)"""
    return P.planes_value(P.rne_planes(x, False, planes), False)


def lsb(x):
    """torch fp64, elementwise: the lowest set bit of x as a power of two (inf where x is zero)"""
    m, e = torch.frexp(x)
    mi = (m.abs() * 2.0 ** 53).long()
    return torch.where(x != 0, torch.ldexp((mi & -mi).double(), e - 53), torch.full_like(x, float("inf")))


def granule(x, dim):
    """the largest power of two that divides every nonzero entry along `dim` (inf where all are zero)"""
    return lsb(x).amin(dim=dim)


def _split_t(x32, planes, trunc=False):
    """torch fp32 -> the fp64 sum of what common.h's split_bf16x2 keeps (or, trunc, of a split that cuts the low 16 bits off)"""
    if trunc:
        cut = lambda y: (y.contiguous().view(torch.int32) & -65536).view(torch.float32)
    else:
        cut = lambda y: y.bfloat16().float()
    hi = cut(x32)
    return hi.double() if planes == 1 else hi.double() + cut(x32 - hi).double()


def _within24(A, Bm, gA, what, nonneg=False):
    """out = A @ Bm per pair: every partial sum is a multiple of granule(row of A) * granule(column of Bm) and stays below sum |terms|.
    gA: the granule of A's rows.  Returns sum |terms|."""
    mag = (A if nonneg else A.abs()) @ Bm.abs()
    g = gA[:, :, None] * granule(Bm, 1)[:, None, :]
    ok = torch.isfinite(g)
    ratio = torch.where(ok, mag / torch.where(ok, g, torch.ones_like(g)), torch.zeros_like(g))
    assert float(ratio.max()) < 2.0 ** 24, f"{what}: a partial sum leaves 24 bits ({float(ratio.max()):.3g})"
    return mag


def _has_lo(x):
    return x.float().bfloat16().double() != x


# ------------------------------------------------------------------------------------------------ the builder
def _dO_O(g, probe, B, H, ntok, n, planes, narrow, rounded):
    """dO, O as [B, ntok, H, 64] and V's magnitude: see the module docstring"""
    shape = (B, ntok, H)
    b_, q_, h_ = np.meshgrid(np.arange(B), np.arange(ntok), np.arange(H), indexing="ij")
    d1 = (5 * q_ + 3 * h_ + 7 * b_ + n) % 64
    d2 = (d1 + 1 + (q_ + 2 * h_ + b_) % 63) % 64
    sign = lambda shp=shape: np.where(g.integers(0, 2, shp) == 0, 1, -1)
    small = lambda lo, hi: g.integers(lo, hi + 1, shape) * sign()
    wide = lambda: 256 * sign() + (2 * g.integers(0, 64, shape) + 1) * sign()
    full = (B, ntok, H, 64)
    if rounded:
        a1, a2 = (small(9, 15), small(9, 15)) if planes == 1 else (wide(), wide())
        omax, vmax = (63, 15) if planes == 1 else (1023, 3)
        O = g.integers(-omax, omax + 1, full)
    elif planes == 1 or narrow:
        a1, a2 = (small(1, 2), 0 * d1) if probe == "groups" else (small(1, 3), small(1, 3))
        vmax = 15
        O = g.integers(-15, 16, full)
    else:
        a1, a2 = wide(), (0 * d1 if probe == "groups" else small(1, 3))
        vmax = 3
        O = g.integers(-3, 4, full)
        np.put_along_axis(O, d2[..., None], wide()[..., None], axis=-1)      # delta needs O's lo plane
    dO = np.zeros(full)
    np.put_along_axis(dO, d1[..., None], a1[..., None].astype(np.float64), axis=-1)
    np.put_along_axis(dO, d2[..., None], a2[..., None].astype(np.float64), axis=-1)
    return dO, O.astype(np.float64), vmax


def build(probe, B, H, ntok, n=0, s=1, t=0, rot=0, planes=1, lo=None, rounded=False, seed=0) -> BwdCase:
    """One probe.  rounded: the first seed from `seed` on at which some dS rounds away from zero, i.e. differs from its truncation."""
    for sd in range(seed, seed + (64 if rounded else 1)):
        c = _build(probe, B, H, ntok, n, s, t, rot, planes, lo, rounded, sd)
        if not rounded or c.meta["rounds_up"]:
            return c
    raise AssertionError("no seed makes the rounded variant round a dS away from zero")


def _build(probe, B, H, ntok, n, s, t, rot, planes, lo, rounded, seed) -> BwdCase:
    assert probe in PROBES and not (rounded and (probe != "pick" or lo))
    c = P.build("selector" if probe == "pick" else probe, B, H, ntok, n=n, s=s, t=t, rot=rot, planes=planes, lo=lo, seed=seed, expect=False)
    npad = c.npad
    g = np.random.default_rng([seed, 77, B, H, ntok, n, planes, int(rounded)])
    dO, O, vmax = _dO_O(g, probe, B, H, ntok, n, planes, narrow=(probe == "pick" and lo is not None), rounded=rounded)
    V = c.V.copy()                                                       # the pad rows stay the forward's large integers
    V[:, :, :ntok] = g.integers(1, vmax + 1, (B, H, ntok, 64)) * np.where(g.integers(0, 2, (B, H, ntok, 64)) == 0, 1, -1)
    pairs = lambda x: torch.from_numpy(np.ascontiguousarray(x[:, :, :ntok])).reshape(B * H, ntok, 64)          # [pair, row, d], fp64
    rows = lambda x: torch.from_numpy(x).permute(0, 2, 1, 3).reshape(B * H, ntok, 64)                         # ctx layout -> the same
    Qt, Kt, Vt, dOt, Ot = pairs(c.Q), pairs(c.K), pairs(V), rows(dO), rows(O)
    lse = torch.zeros((B * H, ntok), dtype=torch.float64)
    q_idx = torch.arange(ntok)
    sums = {k: torch.zeros((B * H, ntok, 64), dtype=torch.float64) for k in ("dq", "dk", "dv")}
    mags = {k: torch.zeros((B * H, ntok, 64), dtype=torch.float64) for k in ("dq", "dk", "dv")}
    any_lo_ds = rounds_up = False
    T = lambda x: x.transpose(1, 2)
    chunk = max(1, 2 ** 23 // (ntok * ntok))                            # pairs per batch: the [ntok, ntok] matrices stay within 64 MB each
    for g0 in range(0, B * H, chunk):
        sl = slice(g0, g0 + chunk)
        q, k, v, do, o = Qt[sl], Kt[sl], Vt[sl], dOt[sl], Ot[sl]        # do and o are views: written below
        S = q @ T(k)                                                     # exact in fp64: dyadic operands of a few bits
        m = S.amax(dim=2)
        hrel = m[:, :, None] - S
        assert bool((S == S.round()).all()), "scores are integers"
        near = hrel <= P.HMAX
        assert bool((near | (hrel >= P.ZERO_FROM)).all()), "a key is neither weighted nor exactly zero"
        gd = float((granule(q, 1) * granule(k, 1)).min())                # per head dimension: the granule of its products
        assert not math.isfinite(gd) or float((q.abs() @ T(k.abs())).max() + m.abs().max() + 2) / gd < 2.0 ** 24, "a score's partial sum"
        nsel = near.sum(dim=2)
        if probe in ("selector", "pick"):
            assert bool((nsel == 1).all())
            ls = m + (q_idx % 2 if probe == "pick" else 0)
        elif probe == "groups":
            pow2 = ((nsel & (nsel - 1)) == 0) & (torch.where(near, hrel, torch.zeros_like(hrel)) == 0).all(dim=2)
            ls = torch.where(pow2, m + torch.log2(nsel.double()), m + 2)
            do[~pow2] = 0.0
        else:
            ls = m + q_idx % 3
        assert bool((ls == ls.round()).all()) and bool((ls >= m).all()), "lse is an integer at or above the row maximum"
        lse[sl] = ls
        Pm = torch.where(near, torch.exp2(torch.where(near, S - ls[:, :, None], torch.zeros_like(S))), torch.zeros_like(S))
        assert bool((torch.frexp(Pm[near])[0] == 0.5).all()), "a probability is not a power of two"
        if probe in ("selector", "groups"):
            consistent = torch.ones_like(nsel, dtype=torch.bool) if probe == "selector" else pow2
            assert bool((Pm.sum(dim=2)[consistent] == 1.0).all()), "lse is not the log-sum-exp"
            o[consistent] = (Pm @ v)[consistent]
        delta = (do * o).sum(dim=2)
        dP = do @ T(v)
        gd = float((granule(do, 1) * granule(v, 1)).min())
        assert not math.isfinite(gd) or float((do.abs() @ T(v.abs())).max() + delta.abs().max()) / gd < 2.0 ** 24, "a dP partial sum"
        assert float((do.abs() * o.abs()).sum(dim=2).max()) < 2.0 ** 24 and bool((do == do.round()).all()) and bool((o * 4 == (o * 4).round()).all())
        dS = Pm * (dP - delta[:, :, None])
        assert bool((dS.float().double() == dS).all()), "a dS is not an fp32 value"
        dSr = _split_t(dS.float(), planes)
        if rounded:
            rounds_up |= bool((_split_t(dS.float(), planes, trunc=True) != dSr).any())
        else:
            assert bool((dSr == dS).all()), f"a dS leaves the {planes} plane(s)"
        if probe == "selector":
            assert bool((dS == 0).all())
        if planes == 2:
            ds_lo = bool(_has_lo(dSr).any())
            any_lo_ds |= ds_lo
            q_lo, k_lo = _has_lo(q).any(dim=1), _has_lo(k).any(dim=1)    # per pair and head dimension
            assert not (ds_lo and bool(k_lo.any())) and not (ds_lo and bool(q_lo.any())), "a lo x lo product"
            assert not bool((q_lo & k_lo).any()) and not bool(_has_lo(v).any()), "a lo x lo product"        # (P is a power of two)
        gP = torch.where(near, Pm, torch.full_like(Pm, float("inf"))).amin(dim=1)      # a power of two is its own lowest bit
        low = lsb(dSr)
        sums["dv"][sl], mags["dv"][sl] = T(Pm) @ do, _within24(T(Pm), do, gP, "dV", nonneg=True)
        sums["dq"][sl], mags["dq"][sl] = dSr @ k, _within24(dSr, k, low.amin(dim=2), "dQ")
        sums["dk"][sl], mags["dk"][sl] = T(dSr) @ q, _within24(T(dSr), q, low.amin(dim=1), "dK")
    ctx_layout = lambda x: x.reshape(B, H, ntok, 64).permute(0, 2, 1, 3).contiguous().numpy()                 # -> [B, ntok, H, 64]
    out = BwdCase(probe, B, H, ntok, npad, planes, c.Q, c.K, V, ctx_layout(dOt).reshape(B * ntok, H * 64), ctx_layout(Ot).reshape(B * ntok, H * 64),
                  lse.reshape(B, H, ntok).numpy(), {k: ctx_layout(x) for k, x in sums.items()}, {k: ctx_layout(x) for k, x in mags.items()},
                  meta={"lo": lo, "rounded": rounded, "n": n, "pi": c.meta["pi"], "any_lo_ds": any_lo_ds, "dims": c.dims,
                        "rounds_up": rounds_up})
    out.expect = expected_planes(out)
    return out


def expected_planes(c: BwdCase):
    """[planes, B * ntok, 3 * H * 64] int16: RNE planes of 0.125 * sum (dQ), of float32(sum) * float32(ln 2) (dK), of the sum (dV)"""
    dq = c.sums["dq"] * 0.125
    assert (c.sums["dk"].astype(F32).astype(np.float64) == c.sums["dk"]).all()
    dk = (c.sums["dk"].astype(F32) * LN2).astype(np.float64)
    full = np.stack([dq, dk, c.sums["dv"]], axis=2)                      # [B, ntok, 3, H, 64]
    return P.rne_planes(full, False, c.planes).reshape(c.planes, c.B * c.ntok, 3 * c.H * 64)


def dk_exact(c: BwdCase):
    """[B * ntok, H * 64] fp64: the exact product float32(sum) * float32(ln 2) of dK"""
    return (c.sums["dk"].astype(F32).astype(np.float64) * float(LN2)).reshape(c.B * c.ntok, c.H * 64)


def mismatches(c: BwdCase, got):
    """(bool [B * ntok, 3 * H * 64]: where the planes `got` miss the condition, worst dK error / bound): bit equality with c.expect on every
    plane; for dK on hi + lo planes the bound of the module docstring instead (a NaN misses it)."""
    bad = (got != c.expect).any(axis=0)
    worst = 0.0
    if c.planes == 2:
        kc = slice(c.H * 64, 2 * c.H * 64)
        x = dk_exact(c)
        with np.errstate(invalid="ignore"):
            ratio = np.abs(P.planes_value(got[:, :, kc], False) - x) / (P.half_ulp_store(x, False, 2) + 2.0 ** -23 * np.abs(x))
        bad[:, kc] = ~(ratio <= 1.0)
        worst = float(np.nan_to_num(ratio, nan=np.inf, posinf=np.inf).max())
    return bad, worst


def operand_planes(c: BwdCase):
    """int16 planes of the six operands as dinoseg_op_attention_bwd takes them (lse as fp32 [B, H, ntok])"""
    qkv = {k: P.exact_planes(getattr(c, k.upper()), False, c.planes).reshape(c.planes, -1, 64) for k in ("q", "k", "v")}
    return dict(qkv, dO=P.exact_planes(c.dO, False, c.planes), O=P.exact_planes(c.O, False, c.planes), lse=c.lse.astype(F32))


def case_list(shapes, planes=1):
    """[(probe, (B, H, ntok), build keywords)] with a running case number n (-> P.case_dims: consecutive cases rotate through the 64
    dimensions).  Selector: every (s, t) of P.coprime_steps, the lo plane alternating between K and Q~ on hi + lo planes; pick: the far stride
    with a lo plane in K and in Q~ (none on one plane), and the identity with a dS that has to be rounded; groups: two strides; weights: the
    far stride at two code rotations; count.  Long sequences (more than 1024 tokens) take one variant of each."""
    out, n = [], 0
    los = [None] if planes == 1 else ["k", "q"]
    for si, shp in enumerate(shapes):
        ntok = shp[2]
        steps = P.coprime_steps(ntok)
        lean = ntok > 1024
        far = steps[-1]
        variants = {
            "selector": [dict(s=s, t=t, lo=los[(i + si) % len(los)]) for i, (s, t) in enumerate(steps[-1:] if lean else steps)],
            "pick": [dict(s=far[0], t=far[1], lo=lo) for lo in (los[si % len(los):][:1] if lean else los)]
                    + ([] if lean else [dict(s=1, t=0, rounded=True)]),
            "groups": [dict(s=s, t=t) for s, t in (steps[-1:] if lean else steps[:2])],
            "weights": [dict(s=far[0], t=far[1], rot=r) for r in ((0,) if lean else (0, ntok // 3))],
            "count": [dict()],
        }
        for probe in PROBES:
            for kw in variants[probe]:
                out.append((probe, shp, dict(kw, n=n, planes=planes)))
                n += 1
    return out


# ------------------------------------------------------------------------------------------------ fp32 emulation of the three launches
def _split(x, planes, trunc=False):
    """fp32 -> (hi, lo) fp32: common.h split_bf16x2, or (the mutant) the same with the low 16 bits cut off instead of rounded"""
    x = np.ascontiguousarray(x, dtype=F32)
    if trunc:
        cut = lambda y: (np.ascontiguousarray(y, dtype=F32).view(np.uint32) & np.uint32(0xFFFF0000)).view(F32)
    else:
        cut = lambda y: torch.from_numpy(np.ascontiguousarray(y, dtype=F32)).bfloat16().float().numpy()
    hi = cut(x)
    if planes == 1:
        return hi, None
    with np.errstate(invalid="ignore"):
        return hi, cut(x - hi)


def _mm3(acc, ah, al, bh, bl):
    """acc + al.bh + ah.bl + ah.bh in fp32: the kernels' three MFMA chains per product (lo.lo is never multiplied)"""
    with np.errstate(invalid="ignore", over="ignore"):
        if al is not None:
            acc = acc + al @ bh
        if bl is not None:
            acc = acc + ah @ bl
        return acc + ah @ bh


def _exp2(s):
    fin = np.isfinite(s)
    assert (s[fin] == np.round(s[fin])).all()
    with np.errstate(invalid="ignore"):
        return np.where(np.isnan(s), F32(np.nan), P._exp2(np.where(fin, s, np.where(s > 0, 400.0, -400.0))))


def emulate(c: BwdCase, order="natural", mut=None):
    """attn_bwd_prep_kernel, attn_bwd_dq_kernel and attn_bwd_dkv_kernel in fp32 numpy, 64-row tile by tile: -lse and -delta as the initial
    accumulators of the score and dP chains (-inf / 0 on pad queries), P and dS rounded to the planes, hi.hi + hi.lo + lo.hi per product,
    the key mask on the ragged last key tile of the dQ kernel, the dO row clamp of the dK,dV kernel's last query tile (dO is followed by
    NaN rows here, as by a guard band).  order: the tiles in natural or reversed order.  mut: one of MUTANTS.  Returns planes like
    c.expect."""
    assert mut is None or mut in MUTANTS
    B, H, ntok, npad, planes = c.B, c.H, c.ntok, c.npad, c.planes
    two = planes == 2
    pv = lambda x: tuple(a if (i == 0 or two) else None for i, a in enumerate(plane_values(x, planes)))
    (Qh, Ql), (Kh, Kl), (Vh, Vl), (Dh, Dl), (Oh, Ol) = pv(c.Q), pv(c.K), pv(c.V), pv(c.dO), pv(c.O)
    tr = lambda x: None if x is None else x.T
    sub = lambda x, *idx: None if x is None else x[idx]
    # prep
    a, o = (Dh + Dl, Oh + Ol) if two else (Dh, Oh)
    delta = (a * o).reshape(B, ntok, H, 64).sum(axis=-1, dtype=F32).transpose(0, 2, 1)
    neg_lse = np.full((B, H, npad), 0.0 if mut == "padq" else -np.inf, F32)
    neg_lse[:, :, :ntok] = -c.lse.astype(F32)
    neg_delta = np.zeros((B, H, npad), F32)
    if mut != "no_delta":
        neg_delta[:, :, :ntok] = -delta
    nanrows = np.full((64, H * 64), np.nan, F32)
    Dh_g, Dl_g = np.concatenate([Dh, nanrows]), (np.concatenate([Dl, nanrows]) if two else None)
    nt = (ntok + 63) // 64

    def tiles(kernel):
        ts = list(range(nt))[::-1 if order == "reversed" else 1]
        if mut == kernel + "_skip":
            ts.remove(nt - 1)
        if mut == kernel + "_twice":
            ts.append(nt - 1)
        return ts
    split = lambda x: _split(x, planes, trunc=(mut == "trunc"))
    out = np.zeros((B, ntok, 3, H, 64), F32)
    lim = ntok + {"mask+1": 1, "mask-1": -1}.get(mut, 0)
    for b in range(B):
        for h in range(H):
            cols = slice(h * 64, h * 64 + 64)
            rows = slice(b * ntok, (b + 1) * ntok)
            qh, ql, kh, kl, vh, vl = (sub(x, b, h) for x in (Qh, Ql, Kh, Kl, Vh, Vl))
            # dQ: every query of the pair, key tile by key tile
            dq = np.zeros((ntok, 64), F32)
            dh, dl = sub(Dh, rows, cols), sub(Dl, rows, cols)
            for t in tiles("dq"):
                ks = slice(t * 64, t * 64 + 64)
                S = _mm3(neg_lse[b, h, :ntok, None], qh[:ntok], sub(ql, slice(0, ntok)), kh[ks].T, tr(sub(kl, ks)))
                if (t + 1) * 64 > lim:
                    S = np.where((t * 64 + np.arange(64) >= lim)[None, :], F32(-np.inf), S)
                D = _mm3(neg_delta[b, h, :ntok, None], dh, dl, vh[ks].T, tr(sub(vl, ks)))
                with np.errstate(invalid="ignore", over="ignore"):
                    sh, sl = split(D * _exp2(S))
                if mut == "no_ds_lo":
                    sl = None
                dq = _mm3(dq, sh, sl, kh[ks], sub(kl, ks))
            # dK, dV: every key of the pair, query tile by query tile
            dk, dv = np.zeros((64, ntok), F32), np.zeros((64, ntok), F32)
            kk = slice(0, ntok)
            for t in tiles("dkv"):
                r = t * 64 + np.arange(64)
                dr = b * ntok + (r if mut == "noclamp" else np.minimum(r, ntok - 1))
                dth, dtl = Dh_g[dr][:, cols], (Dl_g[dr][:, cols] if two else None)
                S = _mm3(neg_lse[b, h][r][:, None], qh[r], sub(ql, r), kh[kk].T, tr(sub(kl, kk)))
                D = _mm3(neg_delta[b, h][r][:, None], dth, dtl, vh[kk].T, tr(sub(vl, kk)))
                Pm = _exp2(S)
                with np.errstate(invalid="ignore", over="ignore"):
                    ph, pl = _split(Pm, planes)
                    sh, sl = split(D * Pm)
                if mut == "no_ds_lo":
                    sl = None
                dv = _mm3(dv, dth.T, tr(dtl), ph, pl)
                dk = _mm3(dk, qh[r].T, tr(sub(ql, r)), sh, sl)
            ho = {0: 1, 1: 0}.get(h, h) if mut == "swap_heads" else h
            fq, fk = (LN2, F32(0.125)) if mut == "scales" else (F32(0.125), LN2)
            with np.errstate(invalid="ignore", over="ignore"):
                out[b, :, 0, ho], out[b, :, 1, ho], out[b, :, 2, ho] = dq * fq, dk.T * fk, dv.T
    hi, lo = _split(out, planes)
    stack = torch.from_numpy(np.stack([hi] if planes == 1 else [hi, lo])).bfloat16().view(torch.int16).numpy()
    return stack.reshape(planes, B * ntok, 3 * H * 64)


def mutant_applies(mut, B, H, ntok, planes):
    """a pad row exists at every listed shape (none is a multiple of 64); the lo plane of dS exists on two planes, a second head from H = 2"""
    return {"no_ds_lo": planes == 2, "swap_heads": H >= 2}.get(mut, True) and (ntok % 64 != 0 or mut not in ("mask+1", "padq", "noclamp"))
