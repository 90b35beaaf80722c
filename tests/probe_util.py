"""Probe builders and per-element bounds for tests/test_forward_probes_gpu.py and tests/test_gelu_formula_cpu.py.

The fused forward launches (mlp_fused2/3/4.hip, the GELU epilogues of gemm*.hip) round their intermediate results to 16 bits at points
that their own fp32 noise moves, so on random data they can only be held to a bound scaled by the largest output.  A probe isolates one
stage with weights that make every OTHER stage exact (W = 0 with the probe in the bias, 0 / 1 selector matrices, rows of +-1 whose
LayerNorm is exactly +-1, operands that are exact in the 16-bit format): what is left is one stage against fp64, element by element.

Nothing here touches the GPU: the formulas are restated in fp64 numpy, the bounds are derived from the instruction sequences the
kernels run (docstrings below) and are never fitted to an output.
"""
from __future__ import annotations

import math

import numpy as np
import torch

U = 2.0 ** -24                       # unit roundoff of fp32: one correctly rounded operation has relative error <= U
ULP = 2.0 * U                        # one ulp of fp32 relative to the value, at worst: the error taken for v_exp_f32 and v_rcp_f32
D, F = 384, 1536                     # the width and the hidden width of the fused launches (ViT-S)
HT = 32                              # hidden units per tile of the fused launches: 48 tiles, 16 accumulator elements x 2 lane halves each
FP16_MAX = 65504.0


def f32c(x: float) -> float:
    """a constant as the kernel holds it: rounded to fp32"""
    return float(np.float32(x))


# ------------------------------------------------------------------------------------------------ the formulas of common.h in fp64
def gelu_exact(x: np.ndarray) -> np.ndarray:
    """0.5 x (1 + erf(x / sqrt 2)) in fp64, written with erfc (1 + erf(z) = erfc(-z)): no cancellation in the negative tail"""
    t = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * t * torch.erfc(-t / math.sqrt(2.0))).numpy()


_F5, _F3, _F1 = f32c(1.01537542e-3), f32c(-1.06782573e-1), f32c(-2.30111381)


def gelu_fast64(x: np.ndarray) -> np.ndarray:
    """common.h gelu_fast in fp64 with the kernel's fp32 constants: x / (1 + 2^(xc q(xc^2))), xc = clamp(x, -8, 8)"""
    x = np.asarray(x, dtype=np.float64)
    xc = np.clip(x, -8.0, 8.0)
    u = xc * xc
    q = (_F5 * u + _F3) * u + _F1
    return x / (1.0 + np.exp2(q * xc))


_RS2, _AP, _L2E = f32c(0.70710678118654752440), f32c(0.32759112), f32c(1.44269504088896340736)
_A5, _A4, _A3, _A2, _A1 = f32c(1.061405429), f32c(-1.453152027), f32c(1.421413741), f32c(-0.284496736), f32c(0.254829592)


def _erf_parts(x):
    z = np.abs(x) * _RS2
    t = 1.0 / (_AP * z + 1.0)
    pl = (((_A5 * t + _A4) * t + _A3) * t + _A2) * t + _A1
    w = -z * z * _L2E
    return z, t, pl, w


def gelu_erf64(x: np.ndarray) -> np.ndarray:
    """common.h gelu_erf in fp64 with the kernel's fp32 constants (Abramowitz & Stegun 7.1.26; p is held one fp32 step above 0.3275911, see
    common.h).  mlp_fused3.hip restates it as max(x, 0) - |x| (P(t) t / 2) exp(-x^2 / 2) with folded constants: gelu_erf64_fused3."""
    x = np.asarray(x, dtype=np.float64)
    _, t, pl, w = _erf_parts(x)
    pe = pl * t * np.exp2(w)
    return 0.5 * x * np.where(x >= 0.0, 2.0 - pe, pe)


def gelu_erf_grad64(x: np.ndarray) -> np.ndarray:
    """common.h gelu_erf_grad in fp64 with the kernel's fp32 constants: Phi(x) + x phi(x), the same erfc and the same exponential"""
    x = np.asarray(x, dtype=np.float64)
    _, t, pl, w = _erf_parts(x)
    e = np.exp2(w)
    pe = pl * t * e
    return x * f32c(0.39894228040143267794) * e + np.where(x >= 0.0, 1.0 - 0.5 * pe, 0.5 * pe)


def gelu_erf64_fused3(x: np.ndarray) -> np.ndarray:
    """mlp_fused3.hip's restatement in fp64 with the constants it holds: p / sqrt 2 and -log2 e / 2 folded to one fp32 constant each (so the
    exponent has an exact 1 / 2 where common.h squares the rounded 1 / sqrt 2), the polynomial's coefficients halved (exact)."""
    x = np.asarray(x, dtype=np.float64)
    c = float(np.float32(_AP) * np.float32(_RS2))
    k = float(np.float32(-0.5) * np.float32(_L2E))
    t = 1.0 / (c * np.abs(x) + 1.0)
    pl = (((0.5 * _A5 * t + 0.5 * _A4) * t + 0.5 * _A3) * t + 0.5 * _A2) * t + 0.5 * _A1
    return np.maximum(x, 0.0) - np.abs(x) * (pl * t * np.exp2(x * x * k))


# ------------------------------------------------------------------------------------------------ fp32 evaluation noise
def e_eval_fast(x: np.ndarray) -> np.ndarray:
    """Bound on |fp32 evaluation - gelu_fast64(x)|, per element, for the nine-instruction program every kernel runs (common.h, and one
    instruction per MFMA gap in mlp_fused2 / mlp_fused4 / gemm_rs): med3, u = xc xc, two fma, a = q xc, e = v_exp_f32(a), d = 1 + e,
    r = v_rcp_f32(d), g = x r.  Each rounding is taken as relative U = 2^-24, v_exp_f32 and v_rcp_f32 as one ulp (2 U):

        q = fma(fma(c5, u, c3), u, c1):   |dq| <= U (|q| + u |c5 u + c3| + u |2 c5 u + c3|)      outer fma, inner fma, the rounding of u
        a = q xc:                         |da| <= |xc| |dq| + U |a|
        e = 2^a:                          |de| <= e (ln 2 |da| + 2 U)
        d = 1 + e:                        |dd| <= |de| + U d
        g = x rcp(d):                     |dg| <= |g| (|dd| / d + 2 U + U)
    """
    x = np.asarray(x, dtype=np.float64)
    xc = np.clip(x, -8.0, 8.0)
    u = xc * xc
    inner = _F5 * u + _F3
    q = inner * u + _F1
    dq = U * (np.abs(q) + u * np.abs(inner) + u * np.abs(2.0 * _F5 * u + _F3))
    a = q * xc
    da = np.abs(xc) * dq + U * np.abs(a)
    e = np.exp2(a)
    de = e * (math.log(2.0) * da + ULP)
    d = 1.0 + e
    dd = de + U * d
    return np.abs(x / d) * (dd / d + ULP + U)


def e_eval_erf(x: np.ndarray) -> np.ndarray:
    """Bound on |fp32 evaluation - gelu_erf64(x)|, per element, valid for common.h's gelu_erf and for mlp_fused3.hip's restatement:

        z = |x| / sqrt 2, d = fma(p, z, 1), t = v_rcp_f32(d):        |dt| <= 4 U t      (z, the fma, one ulp of the reciprocal)
        P(t) by Horner, four fma:  running error  err <- |t| err + U |partial|  (Higham 5.1),  plus |P'(t)| |dt|
        w = -z z log2 e:                                              |dw| <= 4 U |w|    (z twice, two products)
        E = v_exp_f32(w):                                             |dE| <= E (ln 2 |dw| + 2 U)
        pe = P t E:                                                   rel(pe) <= dP / P + 4 U + ln 2 |dw| + 2 U + 2 U (two products)
        x >= 0:  g = 0.5 x (2 - pe):   |dg| <= 0.5 |x| (pe rel(pe) + U (2 - pe)) + U |g|
        x <  0:  g = 0.5 x pe:         |dg| <= 0.5 |x| pe (rel(pe) + U)
    mlp_fused3.hip computes |x| (P t E / 2) and subtracts it from max(x, 0): the same roundings in another order; the bound takes the larger
    of the two branches' rounding terms for both signs.  Where E underflows (|x| > 14.5) the product is below 2^-126 |x|: added as an absolute
    term."""
    x = np.asarray(x, dtype=np.float64)
    z, t, pl, w = _erf_parts(x)
    dt = 4.0 * U * t
    err = np.zeros_like(x)
    part = np.full_like(x, _A5)
    dp = np.full_like(x, _A5)                    # |P'(t)| bounded by the derivative of the polynomial of absolute coefficients
    for c in (_A4, _A3, _A2, _A1):
        dp = dp * t + np.abs(part)
        part = part * t + c
        err = t * err + U * np.abs(part)
    dpl = err + dp * dt
    E = np.exp2(w)
    rel = dpl / np.abs(pl) + 4.0 * U + math.log(2.0) * 4.0 * U * np.abs(w) + ULP + 2.0 * U
    pe = pl * t * E
    g = np.abs(gelu_erf64(x))
    return 0.5 * np.abs(x) * (pe * (rel + U) + U * (2.0 - np.minimum(pe, 2.0))) + U * g + 2.0 ** -126 * np.abs(x)


# ------------------------------------------------------------------------------------------------ number formats
def tdtype(fp16: bool):
    return torch.float16 if fp16 else torch.bfloat16


def rne(v: np.ndarray, fp16: bool) -> np.ndarray:
    """fp32 values -> the 16-bit format, round to nearest even (torch's CPU conversion), back as fp64"""
    t = torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32))
    return t.to(tdtype(fp16)).to(torch.float64).numpy()


def split(v: np.ndarray, fp16: bool):
    """hi = RNE(v), lo = RNE(v - hi) (v - hi is exact in fp32), both as fp64"""
    v32 = np.asarray(v, dtype=np.float32)
    hi = rne(v32, fp16)
    lo = rne((v32.astype(np.float64) - hi).astype(np.float32), fp16)
    return hi, lo


def half_ulp(mag: np.ndarray, fp16: bool, planes: int) -> np.ndarray:
    """Half an ulp of the stored format at magnitude `mag` (what round-to-nearest may lose).  One plane: 2^(e - 8) for bf16, 2^(max(e, -14) - 11)
    for fp16 (subnormals below 2^-14), e = floor(log2 mag).  hi + lo: 2^-17 mag for bf16 (|v - hi| <= 2^(e - 8), and a residual below that
    bound rounds within 2^-8 2^(e - 9)); 2^-22 mag for fp16 plus 2^-25 for a lo plane in fp16's subnormal range (common.h, split2)."""
    mag = np.maximum(np.asarray(mag, dtype=np.float64), 2.0 ** -140)
    e = np.floor(np.log2(mag))
    if planes == 2:
        return 2.0 ** -22 * mag + 2.0 ** -25 if fp16 else 2.0 ** -17 * mag
    return 2.0 ** (np.maximum(e, -14.0) - 11.0) if fp16 else 2.0 ** (e - 8.0)


def representable(v: torch.Tensor, fp16: bool, planes: int) -> torch.Tensor:
    """fp32 tensor: is each value one number of the format (planes 1) or a sum hi + lo of two (planes 2: lo = RNE(v - hi) leaves nothing)"""
    dt = tdtype(fp16)
    hi = v.to(dt).float()
    if planes == 1:
        return hi == v
    r = v - hi
    return r.to(dt).float() == r


# ------------------------------------------------------------------------------------------------ probe vectors
SPECIAL = [0.0, 2.0 ** -20, -2.0 ** -20, 1e-3, -1e-3, 0.565, -0.7518, 7.99, -7.99, 8.0, -8.0, 8.01, -8.01, 11.0, -11.0, 12.0, -12.0,
           30.0, -30.0, 1e3, -1e3]


def gelu_probe_vectors(seed: int = 7) -> np.ndarray:
    """[4, 1536] fp32 pre-activations.  Vector 0: the special points (eight copies each) and a seeded fill of [-9, 9], permuted over the
    units; vector 1 = -vector 0.  Vector 2: every unit in the upper tail -- [8, 12.5] seeded, with 8, 8.01, 11, 12, 30 and 1e3 sprinkled --
    in a second permutation; vector 3 = -vector 2.  So every hidden unit, that is every (hidden tile, accumulator element, lane half), sees a
    value >= 8 and a value <= -8, and both signs of the general range."""
    g = np.random.default_rng(seed)
    pool = np.concatenate([np.repeat(np.array(SPECIAL), 8), g.uniform(-9.0, 9.0, F - 8 * len(SPECIAL))])
    v0 = pool[g.permutation(F)]
    tails = g.uniform(8.0, 12.5, F)
    tails[g.permutation(F)[:96]] = np.tile(np.array([8.0, 8.01, 11.0, 12.0, 30.0, 1e3]), 16)
    v = np.stack([v0, -v0, tails, -tails]).astype(np.float32)
    assert (v.max(axis=0) >= 8.0).all() and (v.min(axis=0) <= -8.0).all()
    return v


def probe_points() -> np.ndarray:
    """every pre-activation the GELU probes use, as fp64 (the CPU test takes the formulas' errors on them)"""
    return np.unique(gelu_probe_vectors().astype(np.float64))


def tie_probe_vectors(fp16: bool, seed: int = 11) -> np.ndarray:
    """[4, 1536] fp32 values in [8, 64) for the store-rounding probe.  With m = a seeded number of the format and h = half its ulp:
    vector 0 = m + h (an exact tie: even and odd m both occur), 1 = the fp32 neighbour below the tie, 2 = the neighbour above, and
    3 = m + r with r an exact tie of the LO plane (|r| < ulp(m) / 2 with one significant bit more than the format holds)."""
    g = np.random.default_rng(seed)
    bits = 11 if fp16 else 8
    e = g.integers(3, 6, F)                                         # binades [8, 16), [16, 32), [32, 64)
    m = (2.0 ** e) * (1.0 + g.integers(1, 2 ** (bits - 1), F) / 2.0 ** (bits - 1))
    ulp = 2.0 ** (e - (bits - 1))
    tie = (m + 0.5 * ulp).astype(np.float32)
    assert (tie.astype(np.float64) == m + 0.5 * ulp).all()
    k = g.integers(2 ** (bits - 1), 2 ** bits, F)                   # 2 k + 1 has bits + 1 significant bits
    r = ulp * 2.0 ** -(bits + 2) * (2 * k + 1) * np.where(g.integers(0, 2, F) == 0, 1.0, -1.0)
    lo_tie = (m + r).astype(np.float32)
    assert (lo_tie.astype(np.float64) == m + r).all() and (np.abs(r) < 0.5 * ulp).all()
    return np.stack([tie, np.nextafter(tie, np.float32(0.0)), np.nextafter(tie, np.float32(1e9)), lo_tie]).astype(np.float32)


def selector(s: int) -> np.ndarray:
    """W2 [384, 1536] with W2[d, d + 384 s] = 1: output column d is hidden unit d + 384 s, and nothing else"""
    w = np.zeros((D, F), dtype=np.float32)
    w[np.arange(D), np.arange(D) + D * s] = 1.0
    return w


def sign_rows(M: int, seed: int, width: int = D) -> np.ndarray:
    """[M, width] rows of +-1 with width / 2 of each sign, a seeded pattern per row: mean 0 and variance 1 exactly, so with eps = 0,
    gamma = 1 and beta = 0 the LayerNorm of a row is the row."""
    g = np.random.default_rng(seed)
    base = np.concatenate([np.ones(width // 2), -np.ones(width // 2)]).astype(np.float32)
    return np.stack([base[g.permutation(width)] for _ in range(M)])


def exact_in_format(shape, seed: int, fp16: bool, lo: float, hi: float, signed: bool = True) -> np.ndarray:
    """seeded fp32 values that the 16-bit format holds exactly: magnitudes in [lo, hi) with six significant bits (exact in bf16 and fp16,
    and six-bit x six-bit products are exact in fp32)"""
    g = np.random.default_rng(seed)
    v = g.uniform(lo, hi, shape)
    e = np.floor(np.log2(v))
    v = np.round(v / 2.0 ** (e - 5)) * 2.0 ** (e - 5)
    if signed:
        v = v * np.where(g.integers(0, 2, shape) == 0, 1.0, -1.0)
    v = v.astype(np.float32)
    assert (rne(v, fp16) == v.astype(np.float64)).all()
    return v


def sum_bound(abs_terms_sum: np.ndarray, n_terms: int, extra: int = 8) -> np.ndarray:
    """fp32 accumulation of n_terms products (exact or rounded once each) in any order, on MFMAs and in the epilogue:
    |error| <= c U sum |term| with c = 4 sqrt(n) + extra.  (The worst case is (n - 1) U sum |term| (Higham 4.2); rounding errors of a long
    sum behave as a random walk, sqrt(n) U with overwhelming probability, and the factor 4 is that margin -- the same constant form
    tests/test_backward_ops_gpu.py uses.  `extra` covers the bias, the residual add and the final roundings.)"""
    return (4.0 * math.sqrt(n_terms) + extra) * U * abs_terms_sum
