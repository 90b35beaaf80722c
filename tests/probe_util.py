"""Probe builders and per-element bounds for tests/test_forward_probes_gpu.py, tests/test_gemm_probes_gpu.py, tests/test_gemm_probes_cpu.py
and tests/test_gelu_formula_cpu.py.

The fused forward launches (mlp_fused2/3/4.hip, the GELU epilogues of gemm*.hip) round their intermediate results to 16 bits at points
that their own fp32 noise moves, so on random data they can only be held to a bound scaled by the largest output.  A probe isolates one
stage with weights that make every OTHER stage exact (W = 0 with the probe in the bias, 0 / 1 selector matrices, rows of +-1 whose
LayerNorm is exactly +-1, operands that are exact in the 16-bit format): what is left is one stage against fp64, element by element.

Nothing here launches a kernel: the formulas are restated in fp64 numpy, the bounds are derived from the instruction sequences the
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


# ------------------------------------------------------------------------------------------------ shared by the probe files
# (tests/test_forward_probes_gpu.py: the fused launches; tests/test_gemm_probes_gpu.py: the stand-alone GEMMs)
GEMMS = ("gemm-1", "gemm-2", "gemm_big-1", "gemm_big-2", "ln_gemm-1", "ln_gemm-2", "gemm_rs-1", "ln_gemm_rs-1")
GEMM_BIG_OPTION = {"gemm": 0, "gemm_big": 2}      # option "gemm_big" that sends dinoseg_op_gemm / dinoseg_op_qkv_gemm to gemm.hip / gemm_big.hip (other routes: 1, the default)
NAN16 = 0x7FC1        # a NaN in both 16-bit formats: what the pad rows hold before the launch


def planes_of(kind):
    return 2 if kind.endswith("3") or kind.endswith("-2") else 1


def unplane(t, fp16):
    """int16 planes [planes, ...] -> fp64 [planes, ...] on the host"""
    return t.view(tdtype(fp16)).to(torch.float64).cpu().numpy()


def stored(v, fp16, planes, sat=True):
    """the value the format holds for fp32 v: RNE (after the fp16 clamp), or hi + lo"""
    v = np.asarray(v, dtype=np.float32)
    if fp16 and sat:
        v = np.clip(v, -FP16_MAX, FP16_MAX)
    if planes == 1:
        return rne(v, fp16)
    hi, lo = split(v, fp16)
    return hi + lo


def exact_operand(shape, seed, fp16, planes, lo, hi, signed=True):
    """seeded fp32 values the kernel's operand planes hold exactly: six significant bits on one plane; on two planes hi (six bits) + lo (six bits,
    |lo| < ulp(hi) / 4), which is its own hi + lo split.  Returns (value fp64, lo part fp64 -- zero on one plane)."""
    v = exact_in_format(shape, seed, fp16, lo, hi, signed).astype(np.float64)
    if planes == 1:
        return v, np.zeros_like(v)
    g = np.random.default_rng(seed + 1000)
    e = np.floor(np.log2(np.abs(v)))
    m6 = 1.0 + g.integers(0, 32, shape) / 32.0
    lo_part = m6 * 2.0 ** (e - (13 if fp16 else 10)) * np.where(g.integers(0, 2, shape) == 0, 1.0, -1.0)
    full = v + lo_part
    h2, l2 = split(full.astype(np.float32), fp16)
    assert (full.astype(np.float32).astype(np.float64) == full).all() and (h2 == v).all() and (l2 == lo_part).all()
    return full, lo_part


def banded(shape, tile=HT, ntiles=F // HT):
    """mask [384, 1536]: output column d multiplies hidden tile d mod 48 only -- each tile's products stand alone in eight columns, so what one
    k-step loses is not buried under the rounding bound of the other 47"""
    d = np.arange(shape[0])[:, None]
    j = np.arange(shape[1])[None, :]
    return (j // tile) == (d % ntiles)


KSL = 32      # W1 row j is non-zero on the k-slice [32 (j mod 12), 32 (j mod 12) + 32): every slice of fc1's k-loop carries 128 hidden units alone


def block_sparse_w1(rows, seed, width=D):
    """[rows, width]: +-{1, 1.25, 1.5, 1.75} on one 32-wide k-slice per row, zero elsewhere (exact in every format, and so are all partial sums)"""
    g = np.random.default_rng(seed)
    w = np.zeros((rows, width), dtype=np.float32)
    nsl = width // KSL
    for j in range(rows):
        k0 = KSL * (j % nsl)
        w[j, k0:k0 + KSL] = (1.0 + g.integers(0, 4, KSL) / 4.0) * np.where(g.integers(0, 2, KSL) == 0, 1.0, -1.0)
    return w


def ln_fc1_case(M, eps, fp16, planes, rows=F, seed=501, offset=64.0, width=D):
    """X [M, width] of +-1, W1, b1 and the fp64 pre-activation z with its bound.  With eps = 0 the LayerNorm of a row is the row; with eps = 1e-6 it
    is the row times rstd = 1 / sqrt(1 + 1e-6), which one plane rounds back to +-1 and two planes carry to 2^-17 / 2^-22.
    |sum| <= 32 x 1.75 = 56, so with b1 = 64 every z lies in [8, 120]: from 8 on the GELU returns z itself, and half an ulp of bf16 is at most 0.25."""
    X = sign_rows(M, seed, width=width)
    W1 = block_sparse_w1(rows, seed + 1, width=width)
    b1 = np.full(rows, offset, dtype=np.float32)
    prod = X.astype(np.float64) @ W1.astype(np.float64).T
    rstd = 1.0 / math.sqrt(1.0 + eps)
    sabs = np.abs(W1).sum(axis=1).astype(np.float64)
    if planes == 1:
        a, a_err = 1.0, 4.0 * U                                   # RNE(rstd) = 1 in bf16 and fp16; the kernel's fp32 statistics are exact on +-1 rows
    else:
        a, a_err = rstd, (2.0 ** -22 if fp16 else 2.0 ** -17) + 4.0 * U
    z = a * prod + b1.astype(np.float64)[None, :]
    zerr = sum_bound(np.abs(b1).astype(np.float64) + sabs, width)[None, :] + a_err * sabs[None, :]
    return X, W1, b1, z, zerr


# ------------------------------------------------------------------------------------------------ the checks of tests/test_gemm_probes_gpu.py
# (here, so that tests/test_gemm_probes_cpu.py can run them on an fp32 emulation of a correct GEMM and on mutants of it)
LOG2E = 1.4426950408889634
QS = float(np.float32(0.125 * LOG2E))      # the Q scale of the forward: 1 / sqrt(64) times log2 e, as the kernels hold it
FMT_IDS = {False: "bf16", True: "fp16"}
KSTEP = {"gemm": 64, "gemm_big": 32, "gemm_cstat": 64}      # the k-step of a kernel's K loop: BK in gemm.hip, big::BK in gemm_big.hip, a pair of 32-wide k-tiles in gemm_cstat (nk2 = K / 64)
WIDTH = {"gemm": 384, "gemm_big": 384, "ln_gemm": 384, "gemm_rs": 768, "ln_gemm_rs": 768}      # K of probes G2: the kernel's width
LN_ROUTES = ("ln_gemm", "ln_gemm_rs")
EPI_GELU, EPI_RELU = 2, 3                  # (dino_amd.capi, restated: this module does not load the library)


def g2_formats(kind):
    """ln_gemm on two planes is bf16 only (dinoseg_op_ln_gemm)"""
    return (False,) if kind == "ln_gemm-2" else (False, True)


def g2_widths(kind):
    """N: 1536, and for gemm_bstat the edges of gemm_rs_supported (N % 64 == 0, N >= 128, 4 N <= 16 KiB)"""
    return (1536, 128, 192, 4096) if kind.split("-")[0] in ("gemm_rs", "ln_gemm_rs") else (1536,)


def g2_eps(kind):
    return (0.0, 1e-6) if kind.split("-")[0] in LN_ROUTES else (0.0,)


# ReLU where the entry has it (dinoseg_op_gemm; gemm.hip refuses it for one fp16 plane: "the inference epilogues only")
G2_CASES = [(k, f, e) for k in GEMMS for f in g2_formats(k) for e in (EPI_GELU, EPI_RELU)
            if e == EPI_GELU or (k.split("-")[0] in ("gemm", "gemm_big") and (k, f) != ("gemm-1", True))]
G2_MS = (77, 673)
# (kind, heads the kernel's *_supported accepts, formats as (fp16, v_bf16)): dmodel % 128 == 0 in gemm.hip, % 384 in gemm_big.hip, K = 384 in
# gemm_ln*.hip, dmodel = 768 in gemm_rs.hip
QKV_KINDS = [("gemm-1", (2, 6, 12), ((False, 0), (True, 0))), ("gemm-2", (2, 6, 12), ((False, 0), (True, 0), (True, 1))),
             ("gemm_big-1", (6, 12), ((False, 0), (True, 0))), ("gemm_big-2", (6, 12), ((False, 0), (True, 0), (True, 1))),
             ("ln_gemm-1", (6,), ((False, 0), (True, 0))), ("ln_gemm-2", (6,), ((False, 0),)),
             ("gemm_rs-1", (12,), ((False, 0), (True, 0))), ("ln_gemm_rs-1", (12,), ((False, 0), (True, 0)))]
G3_CASES = [(k, H, f, vb) for k, hs, fs in QKV_KINDS for H in hs for f, vb in fs]
G3_SHAPES = ((1, 77), (3, 130), (2, 257))


def v_is_fp16(fp16, planes, v_bf16):
    """V is bf16 on one plane whatever the operand format; on fp16 hi + lo planes it is fp16 unless op_v_bf16 asks for bf16"""
    return bool(fp16 and planes == 2 and not v_bf16)


def within(name, err, bound):
    """|err| <= bound per element (numpy arrays or torch tensors); prints the worst |err| / bound and returns it"""
    bound = bound + 0.0 * err
    assert bool((abs(err) < float("inf")).all()), f"{name}: a result is not finite"
    r = err / bound
    i = int(r.argmax())
    at = tuple(int(x) for x in np.unravel_index(i, tuple(err.shape)))
    w = float(r.reshape(-1)[i])
    print(f"{name}: worst |err| / bound {w:.3f} (|err| {float(err.reshape(-1)[i]):.3e}) at {at}")
    assert bool((err <= bound).all()), (name, at, float(err.reshape(-1)[i]), float(bound.reshape(-1)[i]))
    return w


def accum_reference(A, A_lo, W, W_lo, K):
    """G1: A W^T in fp64 on the operands the kernel multiplies (numpy or torch, [M, K] and [N, K]) without the lo x lo products the two-plane
    kernels leave out, and sum_bound of the K products of each element"""
    return A @ W.T - A_lo @ W_lo.T, sum_bound(abs(A) @ abs(W).T, K)


def add_bound(*terms):
    """4 U (|x| + |b| + ...): a residual, bias or position add is one rounded add and the value the sum starts from or ends in (another)"""
    return 4.0 * U * sum(abs(t) for t in terms)


def check_patch(name, out, ref, bound):
    """out [B, n + 1, N] (NaN before the launch): the CLS rows still NaN, the patch rows within the bound"""
    assert bool((out[:, 0] != out[:, 0]).all()), f"{name}: a CLS row was written"
    return within(name, abs(out[:, 1:] - ref), bound)


def check_stored(name, o, z, zerr, W, fp16, planes):
    """G2: o [planes, M, N] fp64 = the stored planes; their sum is fmt(z) within half_ulp(|z| + zerr) + zerr and one number of the format.
    2 bound <= min |W != 0|: one dropped or duplicated product cannot pass."""
    h = o.sum(axis=0)
    bound = half_ulp(np.abs(z) + zerr, fp16, planes) + zerr
    assert (2.0 * bound <= np.abs(W[W != 0]).min()).all(), float(bound.max())
    w = within(name, np.abs(h - z), bound)
    assert bool(representable(torch.from_numpy(h).float(), fp16, planes).all()), f"{name}: a stored value is not a number of the format"
    return w


def check_qkv(name, q, k, v, z, zerr, fp16, planes, v_fp16, B, ntok, H, qs=QS):
    """G3, test_layernorm_qkv_tails' check: z, zerr [M, 3 dm] (numpy); q, k, v int16 planes [planes, B, H, npad, 64] (torch), NAN16 in the pad rows
    before the launch.  q = fmt(z qs), k = fmt(z), v = fmt_v(z) per element; 2 bound <= 1 (qs for Q) <= min |W != 0|."""
    lay = lambda a: a.reshape(B, ntok, 3, H, 64).transpose(2, 0, 3, 1, 4)
    z, zerr = lay(z), lay(np.broadcast_to(zerr, z.shape))
    top = 0.0
    for nm, t, f16, want, werr in (("q", q, fp16, z[0] * qs, zerr[0] * qs + U * np.abs(z[0] * qs)), ("k", k, fp16, z[1], zerr[1]),
                                   ("v", v, v_fp16, z[2], zerr[2])):
        g = unplane(t, f16)[:, :, :, :ntok].sum(axis=0)
        bound = half_ulp(np.abs(want) + werr, f16, planes) + werr
        assert (2.0 * bound <= (qs if nm == "q" else 1.0)).all(), (nm, float(bound.max()))
        top = max(top, within(f"{name} {nm}", np.abs(g - want), bound))
        assert bool(representable(torch.from_numpy(g).float(), f16, planes).all()), f"{name} {nm}: a stored value is not a number of the format"
        assert bool((t[:, :, :, ntok:] == NAN16).all()), f"{name} {nm}: pad rows were written"
    return top
